// dfm_ss.hip — the state-space pass: a Kalman filter and Rauch-Tung-Striebel
// smoother over the observed entries of M panels of one shape that share the
// parameters (Lambda, sigma^2, A, Q, a0, P0), and the two-step fit of Doz,
// Giannone & Reichlin (2011) on top of dfm_em.  The model, the recursion and
// the return codes are stated in include/dfm.h.
//
//   ss_collapse_kernel   per row t of every panel: C_t, b_t, q_t, n_t, l_t — a
//                        GEMM of [mask | zero-filled panel] against the operands
//                        built from Lambda and sigma^2 on the 64 x 64 fp64 tile
//                        (dfm_tile.h).  Mask and fill are formed from the NaN
//                        pattern while a stage is written to LDS; K = N is split
//                        over workgroups in chunks of SS_KC columns, each chunk's
//                        tile stored on its own.
//   ss_filter_kernel     the recursion forwards, one workgroup per panel, s x s
//                        work in LDS: it adds a row's K chunks in their fixed
//                        order and keeps a_t|t, P_t|t, a_t+1|t, P_t+1|t in the
//                        workspace
//   ss_smoother_kernel   the recursion backwards over that workspace, one
//                        workgroup per panel (a launch of its own: either half
//                        alone keeps its uniform values in registers)
// and the quasi-ML EM on top of them (dfm_ss_em, dfm_ss_fit_ml): every panel of
// the batch then has its own parameter block (a panel stride on the operands,
// 0 for the shared call) and an `active` flag, and an iteration adds
//   ss_smoother_kernel<true>  the smoother, which also sums S11, S10, S00 in
//                        registers, forms the lag-one blocks and writes the
//                        M-step GEMM's operand rows
//   ss_mstep_kernel      the transpose of the collapse: [mask | zero-filled
//                        panel]' against those rows on the same tile, K = T in
//                        chunks of SS_KC rows: S_i, g_i, n_i, q_i per series
//   ss_loadings_kernel   per series lambda_i, sigma^2_i and the next pass's
//                        collapse operands
//   ss_transition_kernel per panel A, Q, the companion matrix, a0 / P0
// and ss_empty_column_kernel looks once, before the first pass, for a column
// of a device-resident panel without an observed entry.
// The mixed-frequency entry points (dfm_ss_smooth_mf, dfm_ss_em_mf,
// dfm_ss_fit_mf) run the same launches at the padded state: the collapse on
// wider operands (a tri(C) | b group per class), ss_filter_kernel<true>, which
// updates once per class, ss_smoother_kernel<., true>, which also emits
// Z_l a_t|T and the low class's moments, and the <true> instantiations of the
// M-step kernels, which read and write a series' own class's columns and
// regress the VAR on its own lags.
// dfm_ss_simulate (dfm_ss_sim.hip) runs the plain smoother's launches through
// ss_smooth_core and draws from what they leave on the device.
// No kernel uses an atomic, and the K splits depend on N and T alone: results
// are bit-identical run to run, and panel b of a batch is bit-identical to a
// call on panel b alone.
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_tile.h"

namespace {

constexpr int SS_KC = 256;                    // panel columns per K chunk (a multiple of 16)

DFM_DEV int ss_offA(int a, int kc) { return a * 16 + (kc ^ (((a >> 1) & 1) << 3)); }   // [a][k]
DFM_DEV int ss_offB(int a, int kc) { return kc * 64 + (a ^ ((kc & 7) << 2)); }         // [k][a]

// Columns of a collapsed row: C_t's lower triangle (ss_tri), b_t, q_t, n_t, l_t.
inline int ss_ncols(int r) { return r * (r + 1) / 2 + r + 3; }

// Tile (blockIdx.x, blockIdx.y % nct) of K chunk blockIdx.y / nct of panel
// blockIdx.z.  X: column-major T x N per panel (ldx, stride).  Wm / Wv: the
// operands of the mask and of the values, Npad x NCP row-major, zero past N
// and past ncols; winv: 1 / sigma^2 (Npad, zero past N); panel b's are pstride
// doubles after panel b - 1's (0: shared).  active: null, or per panel 0 = this
// panel is frozen (the workgroup exits at once).  part: [panel][chunk]
// [Tpad][NCP].  q_t = sum x^2 / sigma^2 is summed beside the MFMA by the tile
// that owns its column cq: thread (k, row group) keeps its four rows' sums over
// the stages, and 64 threads add the 16 k in order.
__global__ __launch_bounds__(256) void ss_collapse_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride,
                                                          int T, int N, const double *__restrict__ Wm,
                                                          const double *__restrict__ Wv,
                                                          const double *__restrict__ winv, int64_t pstride,
                                                          const int *__restrict__ active, int NCP, int nct, int KS,
                                                          int Tpad, int cq, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[4 * 1024];   // mask, value, Wm, Wv images of one stage
  double *lm = lds, *lv = lds + 1024, *lbm = lds + 2048, *lbv = lds + 3072;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int rb = blockIdx.x, cb = blockIdx.y % nct, ks = blockIdx.y / nct, b = blockIdx.z;
  if (active && !active[b]) return;
  Wm += (int64_t)b * pstride;
  Wv += (int64_t)b * pstride;
  winv += (int64_t)b * pstride;
  const int abase = rb * 64, bbase = cb * 64;
  const int Npad = (N + 15) & ~15;
  const int k0 = ks * SS_KC, k1 = min(Npad, k0 + SS_KC);
  const bool own_q = cq >= bbase && cq < bbase + 64;
  const double *Xb = X + (int64_t)b * stride;
  const int kk = tid >> 4, g4 = (tid & 15) * 4;   // this thread's k of a stage, and its four rows / columns
  double acc[8][8];
  tile_zero(acc);
  double qs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int kb = k0; kb < k1; kb += 16) {
    const int n = kb + kk;
    double x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = abase + g4 + i;
      x[i] = (n < N && row < T) ? Xb[(int64_t)n * ldx + row] : NAN;
    }
    const double2 m0 = *reinterpret_cast<const double2 *>(Wm + (int64_t)n * NCP + bbase + g4);
    const double2 m1 = *reinterpret_cast<const double2 *>(Wm + (int64_t)n * NCP + bbase + g4 + 2);
    const double2 v0 = *reinterpret_cast<const double2 *>(Wv + (int64_t)n * NCP + bbase + g4);
    const double2 v1 = *reinterpret_cast<const double2 *>(Wv + (int64_t)n * NCP + bbase + g4 + 2);
    const double wi = winv[n];
    __syncthreads();   // the previous stage's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool obs = !isnan(x[i]);
      const double v = obs ? x[i] : 0.0;
      lm[ss_offA(g4 + i, kk)] = obs ? 1.0 : 0.0;
      lv[ss_offA(g4 + i, kk)] = v;
      if (own_q) qs[i] = fma(v * v, wi, qs[i]);
    }
    const int ob = ss_offB(g4, kk);   // four consecutive columns stay consecutive under the swizzle
    lbm[ob] = m0.x; lbm[ob + 1] = m0.y; lbm[ob + 2] = m1.x; lbm[ob + 3] = m1.y;
    lbv[ob] = v0.x; lbv[ob + 1] = v0.y; lbv[ob + 2] = v1.x; lbv[ob + 3] = v1.y;
    __syncthreads();
    tile_step<ss_offA, ss_offB>(acc, lm, lbm, wr, wc, lane);
    tile_step<ss_offA, ss_offB>(acc, lv, lbv, wr, wc, lane);
  }
  double *out = part + ((int64_t)b * KS + ks) * (int64_t)Tpad * NCP;
  tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
    if (col != cq) out[(int64_t)row * NCP + col] = v;
  });
  if (own_q) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) lds[kk * 64 + g4 + i] = qs[i];
    __syncthreads();
    if (tid < 64) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += lds[k * 64 + tid];
      out[(int64_t)(abase + tid) * NCP + cq] = s;
    }
  }
}

struct SsArgs {
  int T, Tt, r, s, ncols, KS, Tpad, NCP;
  const double *part;                  // [panel][chunk][Tpad][NCP]
  const double *Tm, *Q, *a0, *P0;      // s x s, r x r, s, s x s (row-major)
  int64_t pstride;                     // panel b's Tm, Q, a0, P0 are pstride doubles after panel b - 1's (0: shared)
  const int *active;                   // null, or per panel: 0 = frozen, the workgroup exits at once
  double *ws;                          // per panel: a_t|t (Tt x s), a_t|t-1 (Tt x s), P_t|t, P_t|t-1 (Tt x s x s each)
  double *filt, *smooth, *cov, *ll, *nobs;   // per panel T x r, Tt x r, Tt x r x r, 1, 1 (nullptr: not wanted)
  int *flag;                           // per panel: 1 a P_{t+1|t} not positive definite, 2 a G singular
  double *opnd, *mom;                  // the smoother's moments (ss_smoother_kernel<true>): [panel][T][NCP], [panel][SS_MOM]
  int nw;                              // mixed frequency: the low class's weights w_0..w_{nw-1} (device memory)
  const double *w;
  double *agg;                         // per panel Tt x r, the smoothed aggregate Z_l a_t|T (nullptr: not wanted)
};

// Panel blockIdx.x.  Matrices live in LDS with row stride SS_LS; the rows
// i >= r of the companion matrix are the identity shift, so a product with Tm
// or Tm' runs its dot products on the first r rows only and copies the rest.
// P after the update is symmetrised, P after a prediction and the smoothed P
// are computed on the lower triangle and mirrored.  A row without an observed
// entry (n_t = 0; every row t >= T) leaves a and P as they are.  Every
// workspace element is read back by the thread index that wrote it, in the
// filter and (a launch later) in the smoother.
//
// MF: the mixed-frequency model (include/dfm.h).  A collapsed row then holds
// one tri(C) | b group per class (high, low), then q_t, n_t, l_t and the low
// class's count; the update runs once per class with an observed entry.
template <bool MF>
__global__ __launch_bounds__(256) void ss_filter_kernel(SsArgs g) {
  __shared__ double lds[7 * SS_MAT + 7 * 32 + (MF ? 320 : 160) + 4 + (MF ? 24 : 0)];
  __shared__ int ibad, ipiv;
  double *Tm = lds, *P = Tm + SS_MAT, *W = P + SS_MAT, *GA = W + SS_MAT, *K = GA + SS_MAT, *KC = K + SS_MAT,
         *Qr = KC + SS_MAT;
  double *a = Qr + SS_MAT, *an = a + 32, *d = an + 32, *gv = d + 32, *colj = gv + 32, *rowj = colj + 32,
         *crow = rowj + 64, *sc = crow + (MF ? 320 : 160);   // sc: loglik, log det G, observed count
  double *zl = MF ? sc + 4 : nullptr, *wl = MF ? zl + 16 : nullptr;   // MF: Z_l a and the weights
  double *PZl = K + 16, *Vl = KC + 16;  // MF: P Z_l' (s x r) and Z_l P Z_l' (r x r) in the columns K and KC leave free
  const int tid = threadIdx.x, b = blockIdx.x;
  if (g.active && !g.active[b]) return;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s;
  const int nC = r * (r + 1) / 2, nG = nC + r, cq = MF ? 2 * nG : nG, cn = cq + 1, cl = cq + 2;
  const double *gTm = g.Tm + (int64_t)b * g.pstride, *gQ = g.Q + (int64_t)b * g.pstride,
               *ga0 = g.a0 + (int64_t)b * g.pstride, *gP0 = g.P0 + (int64_t)b * g.pstride;
  double *au = g.ws + (int64_t)b * Tt * (2 * s + 2 * ss), *ap = au + (int64_t)Tt * s, *Pu = ap + (int64_t)Tt * s,
         *Pp = Pu + (int64_t)Tt * ss;
  const double *part = g.part + (int64_t)b * g.KS * (int64_t)g.Tpad * g.NCP;
  const int64_t pstep = (int64_t)g.Tpad * g.NCP;
  for (int e = tid; e < ss; e += 256) {
    const int i = e / s, j = e % s;
    Tm[i * SS_LS + j] = gTm[e];
    P[i * SS_LS + j] = gP0[e];
  }
  for (int e = tid; e < r * r; e += 256) Qr[(e / r) * SS_LS + e % r] = gQ[e];
  if (tid < s) a[tid] = ga0[tid];
  if (tid < 3) sc[tid] = 0.0;
  if (MF && tid < g.nw) wl[tid] = g.w[tid];
  if (tid == 0) ibad = 0;
  __syncthreads();
  // One class's update against Z_c: PZ = P Z_c' (s x r), V = Z_c PZ, z = Z_c a,
  // the class's moments at column co of the row.  n_t, l_t and q_t are sums
  // over both classes: the row's first update brings them to the
  // log-likelihood.  The high class reads P and a in place.
  auto update = [&](const double *PZc, const double *Vc, const double *zc, int co, double nt, bool first) {
    const double *PZ = MF ? PZc : P, *V = MF ? Vc : P, *z = MF ? zc : a, *cr = MF ? crow + co : crow;
    auto C = [&](int i, int j) { return cr[ss_tri(i, j)]; };
    for (int e = tid; e < r * r + r; e += 256) {
      if (e < r * r) {   // G = I + C V beside the identity
        const int i = e / r, j = e % r;
        double v = i == j ? 1.0 : 0.0;
        for (int k = 0; k < r; ++k) v = fma(C(i, k), V[k * SS_LS + j], v);
        GA[i * SS_LS + j] = v;
        GA[i * SS_LS + r + j] = i == j ? 1.0 : 0.0;
      } else {           // d = b - C z
        const int i = e - r * r;
        double v = cr[nC + i];
        for (int k = 0; k < r; ++k) v = fma(-C(i, k), z[k], v);
        d[i] = v;
      }
    }
    __syncthreads();
    dfm::block_gj_inverse(GA, r, SS_LS, colj, rowj, sc + 1, &ipiv, &ibad);
    for (int e = tid; e < s * r + r; e += 256) {
      if (e < s * r) {   // K = PZ G^-1
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int k = 0; k < r; ++k) v = fma(PZ[i * SS_LS + k], GA[k * SS_LS + r + j], v);
        K[i * SS_LS + j] = v;
      } else {           // G^-1 d
        const int i = e - s * r;
        double v = 0.0;
        for (int k = 0; k < r; ++k) v = fma(GA[i * SS_LS + r + k], d[k], v);
        gv[i] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < s * r + s + 1; e += 256) {
      if (e < s * r) {            // K C
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int k = 0; k < r; ++k) v = fma(K[i * SS_LS + k], C(k, j), v);
        KC[i * SS_LS + j] = v;
      } else if (e < s * r + s) {   // a + K d
        const int i = e - s * r;
        double v = a[i];
        for (int k = 0; k < r; ++k) v = fma(K[i * SS_LS + k], d[k], v);
        an[i] = v;
      } else {                    // the class's term of the log-likelihood, with z and V from before the update
        double ba = 0.0, aCa = 0.0, dPg = 0.0;
        for (int i = 0; i < r; ++i) {
          double ca = 0.0, pg = 0.0;
          for (int k = 0; k < r; ++k) {
            ca = fma(C(i, k), z[k], ca);
            pg = fma(V[i * SS_LS + k], gv[k], pg);
          }
          ba = fma(cr[nC + i], z[i], ba);
          aCa = fma(z[i], ca, aCa);
          dPg = fma(d[i], pg, dPg);
        }
        if (!MF || first) {
          sc[0] -= 0.5 * (nt * 1.8378770664093453 + crow[cl] + sc[1] + crow[cq] - 2.0 * ba + aCa - dPg);
          sc[2] += nt;
        } else {
          sc[0] -= 0.5 * (sc[1] - 2.0 * ba + aCa - dPg);
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < ss + s; e += 256) {
      if (e < ss) {   // P - K C PZ'
        const int i = e / s, j = e % s;
        double v = P[i * SS_LS + j];
        for (int k = 0; k < r; ++k) v = fma(-KC[i * SS_LS + k], PZ[j * SS_LS + k], v);
        W[i * SS_LS + j] = v;
      } else {
        a[e - ss] = an[e - ss];
      }
    }
    __syncthreads();
    for (int e = tid; e < ss; e += 256) {
      const int i = e / s, j = e % s;
      P[i * SS_LS + j] = 0.5 * (W[i * SS_LS + j] + W[j * SS_LS + i]);
    }
    __syncthreads();
  };
  // ------------------------------------------------------------ the filter
  for (int t = 0; t < Tt; ++t) {
    if (t < T)
      for (int c = tid; c < g.ncols; c += 256) {
        double v = 0.0;
        for (int k = 0; k < g.KS; ++k) v += part[k * pstep + (int64_t)t * g.NCP + c];
        crow[c] = v;
      }
    __syncthreads();
    const double nt = t < T ? crow[cn] : 0.0;
    if (!MF) {
      if (nt > 0.0) update(P, P, a, 0, nt, true);
    } else if (nt > 0.0) {
      const double nl = crow[cq + 3], nh = nt - nl;
      if (nh > 0.0) update(P, P, a, 0, nt, true);
      if (nl > 0.0) {
        const int nw = g.nw;
        for (int e = tid; e < s * r + r; e += 256) {
          if (e < s * r) {   // P Z_l'
            const int i = e / r, j = e % r;
            double v = 0.0;
            for (int k = 0; k < nw; ++k) v = fma(wl[k], P[i * SS_LS + k * r + j], v);
            PZl[i * SS_LS + j] = v;
          } else {           // Z_l a
            const int i = e - s * r;
            double v = 0.0;
            for (int k = 0; k < nw; ++k) v = fma(wl[k], a[k * r + i], v);
            zl[i] = v;
          }
        }
        __syncthreads();
        for (int e = tid; e < r * r; e += 256) {   // Z_l P Z_l'
          const int i = e / r, j = e % r;
          double v = 0.0;
          for (int k = 0; k < nw; ++k) v = fma(wl[k], PZl[(k * r + i) * SS_LS + j], v);
          Vl[i * SS_LS + j] = v;
        }
        __syncthreads();
        update(PZl, Vl, zl, nG, nt, !(nh > 0.0));
      }
    }
    for (int e = tid; e < ss; e += 256) Pu[(int64_t)t * ss + e] = P[(e / s) * SS_LS + e % s];
    if (tid < s) au[(int64_t)t * s + tid] = a[tid];
    if (g.filt && t < T && tid < r) g.filt[((int64_t)b * T + t) * r + tid] = a[tid];
    if (t == Tt - 1) break;
    for (int e = tid; e < ss + s; e += 256) {   // Tm P and Tm a
      if (e < ss) {
        const int i = e / s, j = e % s;
        double v;
        if (i < r) {
          v = 0.0;
          for (int k = 0; k < s; ++k) v = fma(Tm[i * SS_LS + k], P[k * SS_LS + j], v);
        } else {
          v = P[(i - r) * SS_LS + j];
        }
        W[i * SS_LS + j] = v;
      } else {
        const int i = e - ss;
        double v;
        if (i < r) {
          v = 0.0;
          for (int k = 0; k < s; ++k) v = fma(Tm[i * SS_LS + k], a[k], v);
        } else {
          v = a[i - r];
        }
        an[i] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < ss + s; e += 256) {   // (Tm P) Tm' + Qs on the lower triangle
      if (e < ss) {
        const int i = e / s, j = e % s;
        if (i < j) continue;
        double v;
        if (j < r) {
          v = i < r ? Qr[i * SS_LS + j] : 0.0;
          for (int k = 0; k < s; ++k) v = fma(W[i * SS_LS + k], Tm[j * SS_LS + k], v);
        } else {
          v = W[i * SS_LS + j - r];
        }
        P[i * SS_LS + j] = v;
        P[j * SS_LS + i] = v;
      } else {
        a[e - ss] = an[e - ss];
      }
    }
    __syncthreads();
    for (int e = tid; e < ss; e += 256) Pp[(int64_t)(t + 1) * ss + e] = P[(e / s) * SS_LS + e % s];
    if (tid < s) ap[(int64_t)(t + 1) * s + tid] = a[tid];
  }
  if (tid == 0) {
    if (g.ll) g.ll[b] = sc[0];
    g.nobs[b] = sc[2];
    g.flag[b] = ibad;
  }
}

// The smoother of panel blockIdx.x, backwards over what ss_filter_kernel left
// in the workspace; it ORs its flag into the filter's.
//
// MOM: beside the smoothed rows, what the EM's M-step needs (include/dfm.h),
// over the sample's rows t < T (0-based below):
//   S11 = sum_{t=1..T-1} E_t,  E_t = f_t f_t' + Pff_t|T                 (r x r)
//   S10 = sum_{t=1..T-1} f_t a_{t-1}' + (P_t|T J_{t-1}')[:r]             (r x s)
//   S00 = sum_{t=0..T-2} a_t a_t' + P_t|T                                (s x s)
// each summed from the last row to the first, thread e keeping elements e,
// e + 256, ... in registers (the LDS is full); the lag-one block of the pair
// (t + 1, t) is formed while Ps still holds P_{t+1|T}.  Row t < T of opnd is
// the M-step GEMM's operand: tri(E_t), f_t, 1 (the columns beyond stay zero
// from the host's memset).  mom: S11, S10, S00, a_1|T, P_1|T at SS_M*.
constexpr int SS_M11 = 0, SS_M10 = 256, SS_M00 = 768, SS_MA1 = 1792, SS_MP1 = 1824, SS_MOM = 2848;

// AGG: the mixed-frequency model: also the smoothed aggregate Z_l a_t|T, from
// a while it holds row t, and with MOM the low class's group of the operand
// row, tri(Z_l (a a' + P_t|T) Z_l') | Z_l a, after the high class's, then the 1.
template <bool MOM, bool AGG>
__global__ __launch_bounds__(256) void ss_smoother_kernel(SsArgs g) {
  __shared__ double lds[7 * SS_MAT + 4 * 32 + (MOM ? 32 : 0) + (AGG ? SS_WMAX : 0)];
  __shared__ int ibad;
  double *Tm = lds, *P = Tm + SS_MAT, *B1 = P + SS_MAT, *Lw = B1 + SS_MAT, *Tw = Lw + SS_MAT, *J = Tw + SS_MAT,
         *Ps = J + SS_MAT;
  double *a = Ps + SS_MAT, *an = a + 32, *d = an + 32, *gv = d + 32;
  double *fp = gv + 32;   // MOM: f_{t+1|T}, kept while a moves on to row t
  double *wl = AGG ? fp + (MOM ? 32 : 0) : nullptr;   // AGG: the weights
  const int tid = threadIdx.x, b = blockIdx.x;
  if (g.active && !g.active[b]) return;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s;
  const double *au = g.ws + (int64_t)b * Tt * (2 * s + 2 * ss), *ap = au + (int64_t)Tt * s,
               *Pu = ap + (int64_t)Tt * s, *Pp = Pu + (int64_t)Tt * ss;
  const double *gTm = g.Tm + (int64_t)b * g.pstride;
  double s00[4] = {0.0, 0.0, 0.0, 0.0}, s10[2] = {0.0, 0.0}, lag[2] = {0.0, 0.0}, s11 = 0.0;
  auto emit = [&](int t) {   // a and Ps hold row t's smoothed moments
    if (g.smooth && tid < r) g.smooth[((int64_t)b * Tt + t) * r + tid] = a[tid];
    if (g.cov)
      for (int e = tid; e < r * r; e += 256) g.cov[((int64_t)b * Tt + t) * r * r + e] = Ps[(e / r) * SS_LS + e % r];
    if (AGG && g.agg && tid < r) {
      double v = 0.0;
      for (int k = 0; k < g.nw; ++k) v = fma(wl[k], a[k * r + tid], v);
      g.agg[((int64_t)b * Tt + t) * r + tid] = v;
    }
    if (!MOM || t >= T) return;
    double *row = g.opnd + ((int64_t)b * T + t) * g.NCP;
    const int nC = r * (r + 1) / 2;
    if (tid < r * r) {
      const int i = tid / r, j = tid % r;
      const double v = fma(a[i], a[j], Ps[i * SS_LS + j]);
      if (i >= j) row[ss_tri(i, j)] = v;
      if (t >= 1) s11 += v;
    }
    if (tid < r) row[nC + tid] = a[tid];
    if (tid == 0) row[AGG ? 2 * (nC + r) : nC + r] = 1.0;
    if (AGG && tid < r * r) {   // the low class's group
      const int i = tid / r, j = tid % r, nw = g.nw;
      double fi = 0.0, fj = 0.0, pv = 0.0;
      for (int k = 0; k < nw; ++k) {
        fi = fma(wl[k], a[k * r + i], fi);
        fj = fma(wl[k], a[k * r + j], fj);
        double pk = 0.0;
        for (int k2 = 0; k2 < nw; ++k2) pk = fma(wl[k2], Ps[(k * r + i) * SS_LS + k2 * r + j], pk);
        pv = fma(wl[k], pk, pv);
      }
      if (i >= j) row[nC + r + ss_tri(i, j)] = fma(fi, fj, pv);
      if (j == 0) row[nC + r + nC + i] = fi;
    }
    if (t + 1 < T) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        if (e < ss) s00[q] += fma(a[e / s], a[e % s], Ps[(e / s) * SS_LS + e % s]);
      }
    }
  };
  for (int e = tid; e < ss; e += 256) {
    Tm[(e / s) * SS_LS + e % s] = gTm[e];
    Ps[(e / s) * SS_LS + e % s] = Pu[(int64_t)(Tt - 1) * ss + e];
  }
  if (tid < s) a[tid] = au[(int64_t)(Tt - 1) * s + tid];
  if (AGG && tid < g.nw) wl[tid] = g.w[tid];
  if (tid == 0) ibad = 0;
  __syncthreads();
  emit(Tt - 1);
  for (int t = Tt - 2; t >= 0; --t) {
    for (int e = tid; e < ss; e += 256) {
      P[(e / s) * SS_LS + e % s] = Pu[(int64_t)t * ss + e];
      B1[(e / s) * SS_LS + e % s] = Pp[(int64_t)(t + 1) * ss + e];
    }
    if (tid < s) {
      an[tid] = au[(int64_t)t * s + tid];
      d[tid] = ap[(int64_t)(t + 1) * s + tid];
    }
    __syncthreads();
    dfm::block_spd_inverse(B1, Lw, Lw, Tw, s, SS_LS, &ibad);   // P_{t+1|t}^-1 into Lw
    for (int e = tid; e < ss + s; e += 256) {
      if (e < ss) {
        const int i = e / s, j = e % s;
        double v;
        if (j < r) {   // P_t|t Tm'
          v = 0.0;
          for (int k = 0; k < s; ++k) v = fma(P[i * SS_LS + k], Tm[j * SS_LS + k], v);
        } else {
          v = P[i * SS_LS + j - r];
        }
        Tw[i * SS_LS + j] = v;
        B1[i * SS_LS + j] = Ps[i * SS_LS + j] - B1[i * SS_LS + j];   // P_{t+1|T} - P_{t+1|t}
      } else {
        gv[e - ss] = a[e - ss] - d[e - ss];
      }
    }
    if (MOM && tid < r) fp[tid] = a[tid];
    __syncthreads();
    for (int e = tid; e < ss; e += 256) {   // J = P_t|t Tm' P_{t+1|t}^-1
      const int i = e / s, j = e % s;
      double v = 0.0;
      for (int k = 0; k < s; ++k) v = fma(Tw[i * SS_LS + k], Lw[k * SS_LS + j], v);
      J[i * SS_LS + j] = v;
    }
    __syncthreads();
    for (int e = tid; e < ss + s; e += 256) {
      if (e < ss) {   // J (P_{t+1|T} - P_{t+1|t})
        const int i = e / s, j = e % s;
        double v = 0.0;
        for (int k = 0; k < s; ++k) v = fma(J[i * SS_LS + k], B1[k * SS_LS + j], v);
        Lw[i * SS_LS + j] = v;
      } else {
        const int i = e - ss;
        double v = an[i];
        for (int k = 0; k < s; ++k) v = fma(J[i * SS_LS + k], gv[k], v);
        a[i] = v;
      }
    }
    if (MOM && t + 1 < T) {   // the first r rows of P_{t+1|T} J_t'
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = tid + 256 * q;
        if (e < r * s) {
          const int i = e / s, j = e % s;
          double v = 0.0;
          for (int k = 0; k < s; ++k) v = fma(Ps[i * SS_LS + k], J[j * SS_LS + k], v);
          lag[q] = v;
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < ss; e += 256) {
      const int i = e / s, j = e % s;
      if (i < j) continue;
      double v = P[i * SS_LS + j];
      for (int k = 0; k < s; ++k) v = fma(Lw[i * SS_LS + k], J[j * SS_LS + k], v);
      Ps[i * SS_LS + j] = v;
      Ps[j * SS_LS + i] = v;
    }
    __syncthreads();
    emit(t);
    if (MOM && t + 1 < T) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int e = tid + 256 * q;
        if (e < r * s) s10[q] += fma(fp[e / s], a[e % s], lag[q]);
      }
    }
  }
  if (tid == 0 && ibad) g.flag[b] |= 1;
  if (MOM) {   // a and Ps hold row 0
    double *mom = g.mom + (int64_t)b * SS_MOM;
    if (tid < r * r) mom[SS_M11 + tid] = s11;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (tid + 256 * q < r * s) mom[SS_M10 + tid + 256 * q] = s10[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      if (e < ss) {
        mom[SS_M00 + e] = s00[q];
        mom[SS_MP1 + e] = Ps[(e / s) * SS_LS + e % s];
      }
    }
    if (tid < s) mom[SS_MA1 + tid] = a[tid];
  }
}

// ------------------------------------------------------------ the EM's M-step
// Columns of a series' row of the M-step GEMM: S_i's lower triangle, g_i, n_i, q_i.
constexpr int SS_LB = 32;   // series per workgroup of ss_loadings_kernel

// The transpose of the collapse: tile (blockIdx.x, blockIdx.y % nct) of K chunk
// blockIdx.y / nct of panel blockIdx.z of [mask | zero-filled panel]' (N x T)
// against the smoother's operand rows (T x NCP): the mask meets tri(E_t) and
// the 1 (S_i, n_i), the values meet f_t (g_i).  K = T is contiguous in the
// column-major panel: a thread stages four series at one t, sixteen
// consecutive t side by side.  q_i = sum x^2 is summed beside the MFMA as q_t
// is in the collapse.  pm: [panel][chunk][Nr][NCP], Nr = 64 gridDim.x.
// MF: the operand row has a tri | f group per class: the value columns are two
// ranges, and n_i, q_i follow the second group.
template <bool MF>
__global__ __launch_bounds__(256) void ss_mstep_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride, int T,
                                                       int N, const double *__restrict__ opnd,
                                                       const int *__restrict__ active, int r, int NCP, int nct, int KS,
                                                       double *__restrict__ pm) {
  __shared__ __attribute__((aligned(16))) double lds[4 * 1024];
  double *lm = lds, *lv = lds + 1024, *lbm = lds + 2048, *lbv = lds + 3072;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int rb = blockIdx.x, cb = blockIdx.y % nct, ks = blockIdx.y / nct, b = blockIdx.z;
  if (!active[b]) return;
  const int abase = rb * 64, bbase = cb * 64, Nr = 64 * gridDim.x;
  const int nC = r * (r + 1) / 2, nG = nC + r, cn = MF ? 2 * nG : nG, cq = cn + 1;
  const int Tpad = (T + 15) & ~15;
  const int k0 = ks * SS_KC, k1 = min(Tpad, k0 + SS_KC);
  const bool own_q = cq >= bbase && cq < bbase + 64;
  const double *Xb = X + (int64_t)b * stride, *Ob = opnd + (int64_t)b * T * NCP;
  const int ka = tid & 15, ga = (tid >> 4) * 4;   // the panel's stage: this thread's t and its four series
  const int kk = tid >> 4, g4 = (tid & 15) * 4;   // the operand's stage: this thread's t and its four columns
  double acc[8][8];
  tile_zero(acc);
  double qs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int kb = k0; kb < k1; kb += 16) {
    double x[4], o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = abase + ga + i;
      x[i] = (col < N && kb + ka < T) ? Xb[(int64_t)col * ldx + kb + ka] : NAN;
      o[i] = kb + kk < T ? Ob[(int64_t)(kb + kk) * NCP + bbase + g4 + i] : 0.0;
    }
    __syncthreads();   // the previous stage's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool obs = !isnan(x[i]);
      const double v = obs ? x[i] : 0.0;
      lm[ss_offA(ga + i, ka)] = obs ? 1.0 : 0.0;
      lv[ss_offA(ga + i, ka)] = v;
      if (own_q) qs[i] = fma(v, v, qs[i]);
      const int c = bbase + g4 + i;
      const bool fcol = (c >= nC && c < nG) || (MF && c >= nG + nC && c < 2 * nG);
      lbm[ss_offB(g4 + i, kk)] = fcol ? 0.0 : o[i];
      lbv[ss_offB(g4 + i, kk)] = fcol ? o[i] : 0.0;
    }
    __syncthreads();
    tile_step<ss_offA, ss_offB>(acc, lm, lbm, wr, wc, lane);
    tile_step<ss_offA, ss_offB>(acc, lv, lbv, wr, wc, lane);
  }
  double *out = pm + ((int64_t)b * KS + ks) * (int64_t)Nr * NCP;
  tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
    if (col != cq) out[(int64_t)row * NCP + col] = v;
  });
  if (own_q) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) lds[ka * 64 + ga + i] = qs[i];
    __syncthreads();
    if (tid < 64) {
      double s = 0.0;
      for (int k = 0; k < 16; ++k) s += lds[k * 64 + tid];
      out[(int64_t)(abase + tid) * NCP + cq] = s;
    }
  }
}

// Panel blockIdx.x of a device-resident batch: the first column without an
// observed entry into empty[panel], -1 when every column has one (the host
// makes this check itself for a host batch).  A thread walks down its columns
// and leaves each at its first observed entry.
__global__ __launch_bounds__(256) void ss_empty_column_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride,
                                                              int T, int N, int *__restrict__ empty) {
  __shared__ int first[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const double *Xb = X + (int64_t)b * stride;
  int f = N;
  for (int i = tid; i < N && f == N; i += 256) {
    int t = 0;
    while (t < T && isnan(Xb[(int64_t)i * ldx + t])) ++t;
    if (t == T) f = i;
  }
  first[tid] = f;
  __syncthreads();
  if (tid == 0) {
    int c = N;
    for (int k = 0; k < 256; ++k) c = min(c, first[k]);
    empty[b] = c < N ? c : -1;
  }
}

// Panel b's parameter block (ss_block below), as the kernels address it.
struct SsBlock {
  int64_t stride, oWm, oWv, owi, oTm, oQ, oa0, oP0, oL, osig;
};

// Series blockIdx.x * SS_LB + threadIdx.x of panel blockIdx.y: the K chunks of
// its row added in their order, lambda_i = S_i^-1 g_i by a Cholesky in the
// thread's own LDS column, sigma^2_i = (q_i - lambda_i'g_i) / n_i, and the next
// pass's operands of the collapse.  status ([panel][N]): 0, or 1 S_i not
// positive definite, 2 sigma^2_i not positive, 3 no observed entry — the
// parameters of such a series are left as they were.
// MF: low[i] names the series' class; it reads that class's group of its row
// and writes the collapse operands at that class's columns.
template <bool MF>
__global__ __launch_bounds__(SS_LB) void ss_loadings_kernel(const double *__restrict__ pm, int N, int Nr, int r, int NCP,
                                                            int KS, const int *__restrict__ active, SsBlock L,
                                                            double *__restrict__ par, int *__restrict__ status,
                                                            const uint8_t *__restrict__ low) {
  __shared__ double w[(SS_RMAX * (SS_RMAX + 1) / 2 + 2 * SS_RMAX) * SS_LB];
  const int tid = threadIdx.x, i = blockIdx.x * SS_LB + tid, b = blockIdx.y;
  if (!active[b] || i >= N) return;
  const int nC = r * (r + 1) / 2, cn = nC + r;
  const int co = MF && low[i] ? cn : 0, ccn = MF ? 2 * cn : cn, cq = ccn + 1;   // the group, n_i and q_i in the row
  auto W = [&](int e) -> double & { return w[e * SS_LB + tid]; };
  const double *row = pm + ((int64_t)b * KS * Nr + i) * NCP;
  const int64_t kstep = (int64_t)Nr * NCP;
  auto chunks = [&](int c) {
    double v = 0.0;
    for (int k = 0; k < KS; ++k) v += row[k * kstep + c];
    return v;
  };
  for (int c = 0; c < cn; ++c) W(c) = chunks(co + c);
  const double n = chunks(ccn), q = chunks(cq);
  bool bad = false;
  for (int j = 0; j < r; ++j) {
    double d = W(ss_tri(j, j));
    for (int k = 0; k < j; ++k) d -= W(ss_tri(j, k)) * W(ss_tri(j, k));
    if (!(d > 0.0) || isinf(d)) {
      bad = true;
      d = 1.0;
    }
    d = sqrt(d);
    W(ss_tri(j, j)) = d;
    for (int a = j + 1; a < r; ++a) {
      double v = W(ss_tri(a, j));
      for (int k = 0; k < j; ++k) v -= W(ss_tri(a, k)) * W(ss_tri(j, k));
      W(ss_tri(a, j)) = v / d;
    }
  }
  const int y = cn;   // lambda_i, after the two triangular solves
  for (int a = 0; a < r; ++a) {
    double v = W(nC + a);
    for (int k = 0; k < a; ++k) v -= W(ss_tri(a, k)) * W(y + k);
    W(y + a) = v / W(ss_tri(a, a));
  }
  for (int a = r - 1; a >= 0; --a) {
    double v = W(y + a);
    for (int k = a + 1; k < r; ++k) v -= W(ss_tri(k, a)) * W(y + k);
    W(y + a) = v / W(ss_tri(a, a));
  }
  double lg = 0.0;
  for (int a = 0; a < r; ++a) lg = fma(W(y + a), W(nC + a), lg);
  const double v = (q - lg) / n;
  const int st = !(n > 0.0) ? 3 : bad ? 1 : (!(v > 0.0) || isinf(v)) ? 2 : 0;
  status[(int64_t)b * N + i] = st;
  if (st) return;
  double *P = par + (int64_t)b * L.stride;
  double *wm = P + L.oWm + (int64_t)i * NCP, *wv = P + L.oWv + (int64_t)i * NCP;
  for (int a = 0; a < r; ++a) {
    const double la = W(y + a);
    for (int c = 0; c <= a; ++c) wm[co + ss_tri(a, c)] = la * W(y + c) / v;
    wv[co + nC + a] = la / v;
    P[L.oL + (int64_t)a * N + i] = la;
  }
  wm[ccn + 2] = log(v);
  P[L.owi + i] = 1.0 / v;
  P[L.osig + i] = v;
}

// Panel blockIdx.x: A = S10 S00^-1, Q = (S11 - A S10') / (T - 1) symmetrised,
// A into the companion matrix's first r rows, and (update_init) a0 <- a_1|T,
// P0 <- P_1|T.  It also reduces the series' status to the panel's M-step flag
// (1 an S_i, 2 a sigma^2_i, 4 an empty column, 8 S00) and the first such column.
// MF: the regression runs on the leading rp block of S00 and S10 (the VAR's
// own lags); the companion matrix's columns beyond stay zero.
template <bool MF>
__global__ __launch_bounds__(256) void ss_transition_kernel(const double *__restrict__ mom, int T, int N, int r, int s, int rp,
                                                            int update_init, const int *__restrict__ active, SsBlock L,
                                                            double *__restrict__ par, const int *__restrict__ status,
                                                            int *__restrict__ mflag, int *__restrict__ mcol) {
  __shared__ double lds[6 * SS_MAT];
  __shared__ int first[256];
  __shared__ int ibad;
  double *S00 = lds, *Si = S00 + SS_MAT, *Lw = Si + SS_MAT, *Tw = Lw + SS_MAT, *S10 = Tw + SS_MAT, *Am = S10 + SS_MAT;
  const int tid = threadIdx.x, b = blockIdx.x, ss = s * s;
  if (!active[b]) return;
  const double *m = mom + (int64_t)b * SS_MOM;
  double *P = par + (int64_t)b * L.stride;
  const int n = MF ? rp : s;
  for (int e = tid; e < n * n; e += 256) S00[(e / n) * SS_LS + e % n] = m[SS_M00 + (e / n) * s + e % n];
  for (int e = tid; e < r * n; e += 256) S10[(e / n) * SS_LS + e % n] = m[SS_M10 + (e / n) * s + e % n];
  int f = N;
  for (int i = tid; i < N; i += 256)
    if (status[(int64_t)b * N + i] && i < f) f = i;
  first[tid] = f;
  if (tid == 0) ibad = 0;
  __syncthreads();
  dfm::block_spd_inverse(S00, Si, Lw, Tw, n, SS_LS, &ibad);
  for (int e = tid; e < r * n; e += 256) {
    const int i = e / n, j = e % n;
    double v = 0.0;
    for (int k = 0; k < n; ++k) v = fma(S10[i * SS_LS + k], Si[k * SS_LS + j], v);
    Am[i * SS_LS + j] = v;
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += 256) {
    const int i = e / r, j = e % r;
    double v = m[SS_M11 + e];
    for (int k = 0; k < n; ++k) v = fma(-Am[i * SS_LS + k], S10[j * SS_LS + k], v);
    Lw[i * SS_LS + j] = v / (double)(T - 1);
  }
  __syncthreads();
  if (!ibad) {
    for (int e = tid; e < r * r; e += 256) {
      const int i = e / r, j = e % r;
      P[L.oQ + e] = 0.5 * (Lw[i * SS_LS + j] + Lw[j * SS_LS + i]);
    }
    for (int e = tid; e < r * n; e += 256) P[L.oTm + (e / n) * s + e % n] = Am[(e / n) * SS_LS + e % n];
    if (update_init) {
      for (int e = tid; e < ss; e += 256) P[L.oP0 + e] = m[SS_MP1 + e];
      if (tid < s) P[L.oa0 + tid] = m[SS_MA1 + tid];
    }
  }
  if (tid == 0) {
    int c = N;
    for (int k = 0; k < 256; ++k) c = min(c, first[k]);
    int fl = ibad ? 8 : 0;
    if (c < N) {
      const int st = status[(int64_t)b * N + c];
      fl |= st == 3 ? 4 : st == 2 ? 2 : 1;
    }
    mflag[b] = fl;
    mcol[b] = c < N ? c : -1;
  }
}

}  // namespace

int dfm::ss_param_error(dfm_ctx *ctx, const char *who, int rc, int64_t where) {
  switch (rc) {
    case SS_E_LIMIT: return fail(ctx, rc, "%s: the state-space pass serves 1 <= r <= 16, 1 <= p <= 8, r p <= 32", who);
    case SS_E_SIGMA:
      return fail(ctx, rc, "%s: the idiosyncratic variance of column %lld (0-based) is not positive", who,
                  (long long)where);
    case SS_E_VAR: return fail(ctx, rc, "%s: the VAR needs T - p > r p rows and a non-singular Xl'Xl", who);
    case SS_E_NAN: return fail(ctx, rc, "%s: NaN in Lambda, sigma^2, A, Q, a0 or P0", who);
    case SS_E_SINGULAR: return fail(ctx, rc, "%s: Q is not positive definite", who);
    case SS_E_EXPLOSIVE: return fail(ctx, rc, "%s: the VAR is not stationary (the doubling iteration did not converge)", who);
  }
  return fail(ctx, rc, "%s: bad arguments", who);
}

namespace {

// A parameter block: the collapse's operands Wm, Wv (Npad x NCP row-major) and
// winv (Npad), the companion matrix, Q (row-major), a0 (32), P0 (row-major),
// then Lambda (N x r column-major) and sigma^2 (N) as the caller gave them.
// The stride is even: the collapse reads Wm and Wv as double2.
SsBlock ss_block(int N, int r, int s, int NCP) {
  const int64_t Npad = (N + 15) & ~15, ss = (int64_t)s * s;
  SsBlock B;
  B.oWm = 0;
  B.oWv = B.oWm + Npad * NCP;
  B.owi = B.oWv + Npad * NCP;
  B.oTm = B.owi + Npad;
  B.oQ = B.oTm + ss;
  B.oa0 = B.oQ + (int64_t)r * r;
  B.oP0 = B.oa0 + 32;
  B.oL = B.oP0 + ss;
  B.osig = B.oL + (int64_t)N * r;
  B.stride = (B.osig + N + 1) & ~(int64_t)1;
  return B;
}

// The block of checked parameters; a null P0 is the stationary covariance
// (SS_E_EXPLOSIVE when the doubling iteration does not converge).
// low (mixed frequency): a series' tri(C) | b columns are its class's group
// (the low class's follows the high class's), and the column after l_t counts
// the low class.
int ss_fill_block(const SsParams &pr, int N, int NCP, const SsBlock &B, double *hp, const uint8_t *low = nullptr) {
  const int r = pr.r, p = pr.p, s = r * p, nC = r * (r + 1) / 2, nG = nC + r, cq = low ? 2 * nG : nG;
  std::fill(hp, hp + B.stride, 0.0);
  for (int i = 0; i < N; ++i) {
    const double v = pr.sigma2[i];
    const int co = low && low[i] ? nG : 0;
    double *wm = &hp[B.oWm + (size_t)i * NCP], *wv = &hp[B.oWv + (size_t)i * NCP];
    for (int a = 0; a < r; ++a) {
      const double la = pr.L[(size_t)a * N + i];
      for (int c = 0; c <= a; ++c) wm[co + ss_tri(a, c)] = la * pr.L[(size_t)c * N + i] / v;
      wv[co + nC + a] = la / v;
    }
    wm[cq + 1] = 1.0;
    wm[cq + 2] = log(v);
    if (co) wm[cq + 3] = 1.0;
    hp[B.owi + i] = 1.0 / v;
  }
  ss_companion(pr.A, r, p, &hp[B.oTm]);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) hp[B.oQ + i * r + j] = pr.Q[(size_t)j * r + i];
  if (pr.a0) std::copy(pr.a0, pr.a0 + s, &hp[B.oa0]);
  if (pr.P0) {
    for (int i = 0; i < s; ++i)
      for (int j = 0; j < s; ++j) hp[B.oP0 + i * s + j] = pr.P0[(size_t)j * s + i];
  } else if (int rc = ss_stationary_cov(pr.A, pr.Q, r, p, &hp[B.oP0])) {
    return rc;
  }
  std::copy(pr.L, pr.L + (size_t)N * r, &hp[B.oL]);
  std::copy(pr.sigma2, pr.sigma2 + N, &hp[B.osig]);
  return 0;
}

}  // namespace

// The smoother over M panels (layout of dfm_mc).  Outputs host, any nullptr.
// mf: the mixed-frequency model (checked; pr is then the padded state's: p =
// max(p, n_w), A = [A 0]) with its smoothed aggregate agg; null: the plain model.
// after (M = 1): called once the panel's launches are done and checked, with
// what they left on the device (dfm_ss_simulate draws from it); who_plain names
// the plain model's caller in the messages.
int dfm::ss_smooth_core(dfm_ctx *ctx, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx, int64_t stride,
                        bool dev, const SsParams &pr, int h, double *filt, double *smooth, double *cov, double *loglik,
                        int64_t *nobs, const dfm_ss_mf *mf, double *agg, SsAfter *after, const char *who_plain) {
  const char *who = mf ? "dfm_ss_smooth_mf" : who_plain;
  if (M < 0 || h < 0 || h > (1 << 20)) return fail(ctx, -2, "%s: bad arguments", who);
  int64_t where = -1;
  int rc = ss_check_params(N64, pr.r, pr.p, pr.L, pr.sigma2, pr.A, pr.Q, pr.a0, pr.P0, &where);
  if (rc) return ss_param_error(ctx, who, rc, where);
  if (M == 0) return 0;
  if (!X || T64 < 1 || N64 < 1 || ldx < T64 || stride < ldx * N64) return fail(ctx, -2, "%s: bad panel layout", who);
  if (T64 + h > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "panel too large");
  const int T = (int)T64, N = (int)N64, r = pr.r, p = pr.p, s = r * p, ss = s * s, Tt = T + h;
  const int cq = (mf ? 2 : 1) * (r * (r + 1) / 2 + r);
  const int ncols = mf ? cq + 4 : ss_ncols(r), nct = (ncols + 63) / 64, NCP = nct * 64, Npad = (N + 15) & ~15;
  const int nrt = (T + 63) / 64, Tpad = nrt * 64, KS = (Npad + SS_KC - 1) / SS_KC;
  // ---- the shared parameters: operands of the collapse, companion form, Q, a0, P0, then the weights
  const SsBlock B = ss_block(N, r, s, NCP);
  const size_t oWm = B.oWm, oWv = B.oWv, owi = B.owi, oTm = B.oTm, oQ = B.oQ, oa0 = B.oa0, oP0 = B.oP0,
               ow = (size_t)B.stride, total = ow + (mf ? SS_WMAX : 0);
  std::vector<double> hp(total);
  if ((rc = ss_fill_block(pr, N, NCP, B, hp.data(), mf ? mf->low : nullptr)))
    return ss_param_error(ctx, who, rc, -1);
  if (mf) std::copy(mf->w, mf->w + mf->n_w, &hp[ow]);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  StreamBuf dpar;
  HIPCHK(ctx, dpar.alloc(total * 8, st));
  double *dp = (double *)dpar.p;
  HIPCHK(ctx, hipMemcpyAsync(dp, hp.data(), total * 8, hipMemcpyHostToDevice, st));
  // ---- panels per pass: the collapsed rows and the recursion's workspace, about half a GB at the most
  const size_t per_part = (size_t)KS * Tpad * NCP, per_ws = (size_t)Tt * (2 * (size_t)s + 2 * (size_t)ss),
               per_out = (size_t)T * r + (size_t)Tt * r + (size_t)Tt * r * r + 2 + (agg ? (size_t)Tt * r : 0);
  const size_t per = (per_part + per_ws + per_out) * 8;
  const int64_t mb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, 65535), (int64_t)(((size_t)1 << 29) / per)));
  StreamBuf dwork, dx, dflag;
  HIPCHK(ctx, dwork.alloc((size_t)mb * per, st));
  HIPCHK(ctx, dflag.alloc((size_t)mb * 4, st));
  const int64_t span_max = (mb - 1) * stride + ldx * (int64_t)(N - 1) + T;
  if (!dev) HIPCHK(ctx, dx.alloc((size_t)span_max * 8, st));
  double *w = (double *)dwork.p;
  double *part = w, *ws = part + (size_t)mb * per_part, *dfilt = ws + (size_t)mb * per_ws,
         *dsm = dfilt + (size_t)mb * T * r,
         *dcov = dsm + (size_t)mb * Tt * r, *dll = dcov + (size_t)mb * Tt * r * r, *dn = dll + mb, *dagg = dn + mb;
  std::vector<int> hflag((size_t)mb);
  std::vector<double> hn((size_t)mb);
  for (int64_t c0 = 0; c0 < M; c0 += mb) {
    const int64_t n = std::min(mb, M - c0);
    const double *src = X + c0 * stride;
    if (!dev) {
      const int64_t span = (n - 1) * stride + ldx * (int64_t)(N - 1) + T;
      HIPCHK(ctx, hipMemcpyAsync(dx.p, src, (size_t)span * 8, hipMemcpyHostToDevice, st));
      src = (const double *)dx.p;
    }
    {
      Scope sc(ctx, DFM_KC_STATS);
      hipLaunchKernelGGL(ss_collapse_kernel, dim3(nrt, nct * KS, (unsigned)n), dim3(256), 0, st, src, ldx, stride, T, N,
                         dp + oWm, dp + oWv, dp + owi, (int64_t)0, (const int *)nullptr, NCP, nct, KS, Tpad, cq, part);
    }
    HIPCHK(ctx, hipGetLastError());
    {
      Scope sc(ctx, DFM_KC_MISC);
      SsArgs g{T, Tt, r, s, ncols, KS, Tpad, NCP, part, dp + oTm, dp + oQ, dp + oa0, dp + oP0, 0, nullptr, ws,
               filt ? dfilt : nullptr, smooth ? dsm : nullptr, cov ? dcov : nullptr, dll, dn, (int *)dflag.p,
               nullptr, nullptr, mf ? mf->n_w : 0, dp + ow, agg ? dagg : nullptr};
      if (mf) {
        hipLaunchKernelGGL(ss_filter_kernel<true>, dim3((unsigned)n), dim3(256), 0, st, g);
        hipLaunchKernelGGL((ss_smoother_kernel<false, true>), dim3((unsigned)n), dim3(256), 0, st, g);
      } else {
        hipLaunchKernelGGL(ss_filter_kernel<false>, dim3((unsigned)n), dim3(256), 0, st, g);
        hipLaunchKernelGGL((ss_smoother_kernel<false, false>), dim3((unsigned)n), dim3(256), 0, st, g);
      }
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(hflag.data(), dflag.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hn.data(), dn, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (filt) HIPCHK(ctx, hipMemcpyAsync(filt + c0 * T * r, dfilt, (size_t)n * T * r * 8, hipMemcpyDeviceToHost, st));
    if (smooth) HIPCHK(ctx, hipMemcpyAsync(smooth + c0 * Tt * r, dsm, (size_t)n * Tt * r * 8, hipMemcpyDeviceToHost, st));
    if (cov)
      HIPCHK(ctx, hipMemcpyAsync(cov + c0 * Tt * r * r, dcov, (size_t)n * Tt * r * r * 8, hipMemcpyDeviceToHost, st));
    if (loglik) HIPCHK(ctx, hipMemcpyAsync(loglik + c0, dll, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (agg) HIPCHK(ctx, hipMemcpyAsync(agg + c0 * Tt * r, dagg, (size_t)n * Tt * r * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
      if (hflag[i])
        return fail(ctx, SS_E_SINGULAR, "%s: panel %lld: %s not invertible", who, (long long)(c0 + i),
                    (hflag[i] & 2) ? "a G = I + C_t Pff is" : "a P_{t+1|t} is");
      if (nobs) nobs[c0 + i] = (int64_t)hn[i];
    }
    if (after && M == 1) {
      const SsKept kept{T, Tt, r, s, ncols, KS, Tpad, NCP, part, ws, dp + oTm, dp + oP0,
                        &hp[oTm], &hp[oQ], &hp[oa0], &hp[oP0]};
      if ((rc = after->run(kept))) return rc;
    }
  }
  return 0;
}

namespace {

// The EM over M panels (include/dfm.h).  The panel and the starts go up once;
// per iteration one read-back (logliks and flags) decides which panels stop,
// and the `active` flags go back; the rest crosses the bus at the end.
int ss_em_core(dfm_ctx *ctx, const char *who, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx,
               int64_t stride, bool dev, const dfm_ss_params *starts, int64_t n_start, int max_iter, double tol, bool update_init, int h,
               const dfm_ss_em_out &out, dfm_ss_em_info *info, const dfm_ss_mf *mf = nullptr, int p_var = 0) {
  // mf: the mixed-frequency model (checked): the starts are then the padded state's (p = max(p_var, n_w), A = [A 0]),
  // p_var the VAR's own lag count (out.A is r x r p_var); null: the plain model
  if (ss_em_check_args(X != nullptr, M, T64, N64, ldx, stride, starts != nullptr, n_start))
    return fail(ctx, -2, "%s: bad arguments (T >= 2, n_start 1 or M)", who);
  if (M == 0) return 0;
  const int r = starts[0].r, p = starts[0].p;
  for (int64_t k = 0; k < n_start; ++k) {
    const dfm_ss_params &q = starts[k];
    if (q.r != r || q.p != p) return fail(ctx, -2, "%s: start %lld has another (r, p)", who, (long long)k);
    int64_t where = -1;
    const int rc = ss_em_check_start(N64, q.r, q.p, q.lambda, q.sigma2, q.A, q.Q, q.a0, q.P0, &where);
    if (rc) return ss_param_error(ctx, who, rc, where);
  }
  int64_t ep = -1, ec = -1;
  if (!dev && ss_em_empty_column(X, M, T64, N64, ldx, stride, &ep, &ec))
    return fail(ctx, -2, "%s: panel %lld: column %lld (0-based) has no observed entry", who, (long long)ep, (long long)ec);
  if (T64 + h > (1 << 24) || M > (1 << 30)) return fail(ctx, -2, "panel too large");
  const int T = (int)T64, N = (int)N64, s = r * p, ss = s * s, Tt = T + h, rp = mf ? r * p_var : s;
  const int cq = (mf ? 2 : 1) * (r * (r + 1) / 2 + r);
  const int ncols = mf ? cq + 4 : ss_ncols(r), nct = (ncols + 63) / 64, NCP = nct * 64, Npad = (N + 15) & ~15;
  const int nrt = (T + 63) / 64, Tpad = nrt * 64, KS = (Npad + SS_KC - 1) / SS_KC;
  const int nrn = (N + 63) / 64, Nr = nrn * 64, KT = (((T + 15) & ~15) + SS_KC - 1) / SS_KC;
  const SsBlock B = ss_block(N, r, s, NCP);
  const size_t blk = (size_t)B.stride, tail = blk - (size_t)B.oTm;
  // ---- the starts' blocks
  std::vector<double> hp((size_t)n_start * blk);
  for (int64_t k = 0; k < n_start; ++k) {
    const dfm_ss_params &q = starts[k];
    const SsParams pr{q.r, q.p, q.lambda, q.sigma2, q.A, q.Q, q.a0, q.P0};
    if (int rc = ss_fill_block(pr, N, NCP, B, &hp[(size_t)k * blk], mf ? mf->low : nullptr))
      return ss_param_error(ctx, who, rc, -1);
  }
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  StreamBuf dmf;   // mixed frequency: the weights, then the mask
  const double *dw = nullptr;
  const uint8_t *dlow = nullptr;
  if (mf) {
    HIPCHK(ctx, dmf.alloc(SS_WMAX * 8 + (size_t)N, st));
    double hw[SS_WMAX] = {0.0};
    std::copy(mf->w, mf->w + mf->n_w, hw);
    dw = (const double *)dmf.p;
    dlow = (const uint8_t *)dmf.p + SS_WMAX * 8;
    HIPCHK(ctx, hipMemcpyAsync(dmf.p, hw, sizeof hw, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync((void *)dlow, mf->low, (size_t)N, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // hw leaves scope
  }
  // ---- panels per pass: the half-GB rule of the smoother over everything a panel keeps on the device
  const size_t per_part = (size_t)KS * Tpad * NCP, per_ws = (size_t)Tt * (2 * (size_t)s + 2 * (size_t)ss),
               per_pm = (size_t)KT * Nr * NCP, per_op = (size_t)T * NCP, per_filt = (size_t)T * r,
               per_sm = (size_t)Tt * r, per_cov = (size_t)Tt * r * r, per_agg = mf ? per_sm : 0;
  const size_t per = (per_part + per_ws + per_pm + per_op + per_filt + per_sm + per_cov + per_agg + SS_MOM + blk + 2) * 8 +
                     ((size_t)N + 4) * 4;
  const int64_t mb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(M, 65535), (int64_t)(((size_t)1 << 29) / per)));
  StreamBuf dpar, dwork, dx, dint;
  HIPCHK(ctx, dpar.alloc((size_t)mb * blk * 8, st));
  HIPCHK(ctx, dwork.alloc((size_t)mb * (per_part + per_ws + per_pm + per_op + per_filt + per_sm + per_cov + per_agg + SS_MOM + 2) * 8,
                          st));
  HIPCHK(ctx, dint.alloc((size_t)mb * ((size_t)N + 4) * 4, st));
  const int64_t span_max = (mb - 1) * stride + ldx * (int64_t)(N - 1) + T;
  if (!dev) HIPCHK(ctx, dx.alloc((size_t)span_max * 8, st));
  double *dp = (double *)dpar.p, *part = (double *)dwork.p, *ws = part + (size_t)mb * per_part,
         *pm = ws + (size_t)mb * per_ws, *opnd = pm + (size_t)mb * per_pm, *dfilt = opnd + (size_t)mb * per_op,
         *dsm = dfilt + (size_t)mb * per_filt, *dcov = dsm + (size_t)mb * per_sm, *mom = dcov + (size_t)mb * per_cov,
         *dll = mom + (size_t)mb * SS_MOM, *dn = dll + mb,   // dll, dn adjacent: one read-back
         *dagg = dn + mb;
  int *eflag = (int *)dint.p, *mflag = eflag + mb, *mcol = mflag + mb, *dact = mcol + mb, *status = dact + mb;
  const size_t path_ld = (size_t)max_iter + 1;
  std::vector<double> hll((size_t)2 * mb), prev((size_t)mb), htail;
  std::vector<int> hflag((size_t)3 * mb), act((size_t)mb);
  std::vector<dfm_ss_em_info> inf((size_t)mb);
  if (dev) {   // a column without an observed entry: the host batch was checked before anything went up
    StreamBuf dempty;
    std::vector<int> hempty((size_t)M);
    HIPCHK(ctx, dempty.alloc((size_t)M * 4, st));
    {
      Scope sc(ctx, DFM_KC_MISC);
      hipLaunchKernelGGL(ss_empty_column_kernel, dim3((unsigned)M), dim3(256), 0, st, X, ldx, stride, T, N, (int *)dempty.p);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(hempty.data(), dempty.p, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i < M; ++i)
      if (hempty[i] >= 0)
        return fail(ctx, -2, "%s: panel %lld: column %d (0-based) has no observed entry", who, (long long)i, hempty[i]);
  }
  for (int64_t c0 = 0; c0 < M; c0 += mb) {
    const int64_t n = std::min(mb, M - c0);
    const double *src = X + c0 * stride;
    if (!dev) {
      const int64_t span = (n - 1) * stride + ldx * (int64_t)(N - 1) + T;
      HIPCHK(ctx, hipMemcpyAsync(dx.p, src, (size_t)span * 8, hipMemcpyHostToDevice, st));
      src = (const double *)dx.p;
    }
    for (int64_t i = 0; i < n; ++i)
      HIPCHK(ctx, hipMemcpyAsync(dp + (size_t)i * blk, &hp[(size_t)(n_start == 1 ? 0 : c0 + i) * blk], blk * 8,
                                 hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(opnd, 0, (size_t)n * per_op * 8, st));
    HIPCHK(ctx, hipMemsetAsync(dint.p, 0, (size_t)mb * ((size_t)N + 4) * 4, st));
    std::fill(act.begin(), act.end(), 1);
    HIPCHK(ctx, hipMemcpyAsync(dact, act.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (out.loglik_path)
      std::fill(out.loglik_path + (size_t)c0 * path_ld, out.loglik_path + (size_t)(c0 + n) * path_ld, (double)NAN);
    int64_t nact = n;
    for (int j = 0;; ++j) {
      {
        Scope sc(ctx, DFM_KC_STATS);
        hipLaunchKernelGGL(ss_collapse_kernel, dim3(nrt, nct * KS, (unsigned)n), dim3(256), 0, st, src, ldx, stride, T, N,
                           dp + B.oWm, dp + B.oWv, dp + B.owi, B.stride, (const int *)dact, NCP, nct, KS, Tpad, cq, part);
      }
      HIPCHK(ctx, hipGetLastError());
      {
        Scope sc(ctx, DFM_KC_MISC);
        SsArgs g{T, Tt, r, s, ncols, KS, Tpad, NCP, part, dp + B.oTm, dp + B.oQ, dp + B.oa0, dp + B.oP0, B.stride, dact,
                 ws, dfilt, dsm, dcov, dll, dn, eflag, opnd, mom, mf ? mf->n_w : 0, dw, mf ? dagg : nullptr};
        if (mf) {
          hipLaunchKernelGGL(ss_filter_kernel<true>, dim3((unsigned)n), dim3(256), 0, st, g);
          hipLaunchKernelGGL((ss_smoother_kernel<true, true>), dim3((unsigned)n), dim3(256), 0, st, g);
        } else {
          hipLaunchKernelGGL(ss_filter_kernel<false>, dim3((unsigned)n), dim3(256), 0, st, g);
          hipLaunchKernelGGL((ss_smoother_kernel<true, false>), dim3((unsigned)n), dim3(256), 0, st, g);
        }
      }
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(hll.data(), dll, (size_t)mb * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(hflag.data(), eflag, (size_t)3 * mb * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      for (int64_t i = 0; i < n; ++i) {
        if (!act[i]) continue;
        const long long pb = (long long)(c0 + i);
        const int mf = hflag[(size_t)mb + i], mc = hflag[(size_t)2 * mb + i], ef = hflag[i];
        if (mf & 4)
          return fail(ctx, -2, "%s: panel %lld: column %d (0-based) has no observed entry", who, pb, mc);
        if (mf & 2)
          return fail(ctx, SS_E_SIGMA, "%s: panel %lld, the M-step giving iteration %d: the idiosyncratic variance of "
                      "column %d (0-based) is not positive", who, pb, j, mc);
        if (mf)
          return fail(ctx, SS_E_SINGULAR, "%s: panel %lld, the M-step giving iteration %d: %s not invertible", who, pb, j,
                      (mf & 8) ? "S00 is" : "an S_i is");
        if (ef)
          return fail(ctx, SS_E_SINGULAR, "%s: panel %lld, the E-step of iteration %d: %s not invertible", who, pb, j,
                      (ef & 2) ? "a G = I + C_t Pff is" : "a P_{t+1|t} is");
        const double ll = hll[i];
        if (out.loglik_path) out.loglik_path[(size_t)(c0 + i) * path_ld + j] = ll;
        const double c = j >= 1 ? ss_em_criterion(ll, prev[i]) : (double)NAN;
        const bool conv = j >= 1 && ss_em_converged(c, tol);
        prev[i] = ll;
        if (conv || j == max_iter) {
          act[i] = 0;
          --nact;
          inf[i] = dfm_ss_em_info{j, conv ? 1 : 0, ll, c};
        }
      }
      if (nact == 0) break;
      HIPCHK(ctx, hipMemcpyAsync(dact, act.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
      {
        Scope sc(ctx, DFM_KC_GEMM);
        hipLaunchKernelGGL(mf ? ss_mstep_kernel<true> : ss_mstep_kernel<false>, dim3(nrn, nct * KT, (unsigned)n), dim3(256), 0,
                           st, src, ldx, stride, T, N, (const double *)opnd, (const int *)dact, r, NCP, nct, KT, pm);
      }
      HIPCHK(ctx, hipGetLastError());
      {
        Scope sc(ctx, DFM_KC_OLS);
        hipLaunchKernelGGL(mf ? ss_loadings_kernel<true> : ss_loadings_kernel<false>,
                           dim3((N + SS_LB - 1) / SS_LB, (unsigned)n), dim3(SS_LB), 0, st, (const double *)pm, N, Nr, r, NCP,
                           KT, (const int *)dact, B, dp, status, dlow);
        hipLaunchKernelGGL(mf ? ss_transition_kernel<true> : ss_transition_kernel<false>, dim3((unsigned)n), dim3(256), 0,
                           st, (const double *)mom, T, N, r, s, rp, update_init ? 1 : 0, (const int *)dact, B, dp,
                           (const int *)status, mflag, mcol);
      }
      HIPCHK(ctx, hipGetLastError());
    }
    // ---- the pass's results
    if (out.filtered)
      HIPCHK(ctx, hipMemcpyAsync(out.filtered + c0 * per_filt, dfilt, (size_t)n * per_filt * 8, hipMemcpyDeviceToHost, st));
    if (out.smoothed)
      HIPCHK(ctx, hipMemcpyAsync(out.smoothed + c0 * per_sm, dsm, (size_t)n * per_sm * 8, hipMemcpyDeviceToHost, st));
    if (out.smoothed_cov)
      HIPCHK(ctx, hipMemcpyAsync(out.smoothed_cov + c0 * per_cov, dcov, (size_t)n * per_cov * 8, hipMemcpyDeviceToHost, st));
    if (mf && out.smoothed_agg)
      HIPCHK(ctx, hipMemcpyAsync(out.smoothed_agg + c0 * per_sm, dagg, (size_t)n * per_sm * 8, hipMemcpyDeviceToHost, st));
    htail.resize((size_t)n * tail);
    HIPCHK(ctx, hipMemcpy2DAsync(htail.data(), tail * 8, dp + B.oTm, blk * 8, tail * 8, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hll.data(), dll, (size_t)2 * mb * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
      const double *tl = &htail[(size_t)i * tail];
      auto t = [&](int64_t off) { return tl + (off - B.oTm); };   // the block's offsets, over its tail
      const size_t g = (size_t)(c0 + i);
      if (out.A)
        for (int k = 0; k < rp; ++k)
          for (int a = 0; a < r; ++a) out.A[g * r * rp + (size_t)k * r + a] = t(B.oTm)[a * s + k];
      if (out.Q)
        for (int a = 0; a < r; ++a)
          for (int c = 0; c < r; ++c) out.Q[g * r * r + (size_t)c * r + a] = t(B.oQ)[a * r + c];
      if (out.a0) std::copy(t(B.oa0), t(B.oa0) + s, out.a0 + g * s);
      if (out.P0)
        for (int a = 0; a < s; ++a)
          for (int c = 0; c < s; ++c) out.P0[g * ss + (size_t)c * s + a] = t(B.oP0)[a * s + c];
      if (out.lambda) std::copy(t(B.oL), t(B.oL) + (size_t)N * r, out.lambda + g * N * r);
      if (out.sigma2) std::copy(t(B.osig), t(B.osig) + N, out.sigma2 + g * N);
      if (out.n_observed) out.n_observed[g] = (int64_t)hll[(size_t)mb + i];
      if (info) info[g] = inf[i];
    }
  }
  return 0;
}

int ss_fit_impl(dfm_ctx *ctx, const char *who, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, const dfm_ss_em_spec *ml, double *a0_out,
                double *loglik_path, dfm_ss_em_info *ml_info, const dfm_ss_mf *mf = nullptr, double *agg_out = nullptr);

}  // namespace

extern "C" {

int dfm_ss_stationary_cov(const double *A, const double *Q, int r, int p, double *P0_out) {
  const int rc = ss_check_dims(r, p);
  if (rc) return rc;
  const int s = r * p;
  std::vector<double> P((size_t)s * s);
  const int e = ss_stationary_cov(A, Q, r, p, P.data());
  if (e) return e;
  std::copy(P.begin(), P.end(), P0_out);   // symmetric: row-major == column-major
  return 0;
}

int dfm_ss_smooth(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                  const dfm_ss_params *params, const dfm_ss_spec *spec, double *filtered, double *smoothed,
                  double *smoothed_cov, double *loglik, int64_t *n_observed) {
  if (!ctx) return -1;
  if (!params || !spec) return fail(ctx, -2, "dfm_ss_smooth: bad arguments");
  DeviceShare gate(ctx->device);
  const SsParams pr{params->r, params->p, params->lambda, params->sigma2, params->A, params->Q, params->a0, params->P0};
  return ss_smooth_core(ctx, X, M, T, N, ldx, stride, spec->dev != 0, pr, spec->horizon, filtered, smoothed,
                        smoothed_cov, loglik, n_observed);
}

int dfm_ss_smooth_mf(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *params, const dfm_ss_mf *mf, const dfm_ss_spec *spec, double *filtered,
                     double *smoothed, double *smoothed_cov, double *loglik, int64_t *n_observed,
                     double *smoothed_agg) {
  if (!ctx) return -1;
  if (!params || !spec || !mf || N < 1) return fail(ctx, -2, "dfm_ss_smooth_mf: bad arguments");
  if (!mf->low) return fail(ctx, -2, "dfm_ss_smooth_mf: the mask of low-frequency series is missing");
  if (!ss_mf_any_low(mf->low, N))
    return dfm_ss_smooth(ctx, X, M, T, N, ldx, stride, params, spec, filtered, smoothed, smoothed_cov, loglik, n_observed);
  const int r = params->r, p = params->p;
  const int rc = ss_mf_check(r, p, mf->n_w, mf->w, mf->low);
  if (rc == SS_E_LIMIT)
    return fail(ctx, rc, "dfm_ss_smooth_mf: the mixed-frequency pass serves 1 <= r <= 16, 1 <= p <= 8, 1 <= n_w <= 8, "
                "r max(p, n_w) <= 32");
  if (rc) return fail(ctx, rc, "dfm_ss_smooth_mf: the weights must be finite with w_0 != 0, and r, p, n_w >= 1");
  if (!params->A) return fail(ctx, -2, "dfm_ss_smooth_mf: bad arguments");
  const int L = ss_mf_lags(p, mf->n_w);
  std::vector<double> Apad((size_t)r * r * L);
  ss_mf_pad_A(params->A, r, p, L, Apad.data());
  DeviceShare gate(ctx->device);
  const SsParams pr{r, L, params->lambda, params->sigma2, Apad.data(), params->Q, params->a0, params->P0};
  return ss_smooth_core(ctx, X, M, T, N, ldx, stride, spec->dev != 0, pr, spec->horizon, filtered, smoothed,
                        smoothed_cov, loglik, n_observed, mf, smoothed_agg);
}

int dfm_ss_estimate(dfm_ctx *ctx, const double *Zm, int64_t T, int64_t N, int64_t ldx, const double *F, const double *L,
                    int r, int p, double *sigma_out, double *A_out, double *Q_out, double *P0_out) {
  if (!ctx) return -1;
  int64_t where = -1;
  const int rc = ss_estimate(Zm, T, N, ldx, F, L, r, p, sigma_out, A_out, Q_out, P0_out, &where);
  return rc ? ss_param_error(ctx, "dfm_ss_estimate", rc, where) : 0;
}

int dfm_ss_em(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
              const dfm_ss_params *starts, int64_t n_start, const dfm_ss_em_spec *spec, const dfm_ss_em_out *out,
              dfm_ss_em_info *info) {
  if (!ctx) return -1;
  int max_iter = 0;
  double tol = 0.0;
  if (!spec || !out || ss_em_defaults(spec->max_iter, spec->tol, spec->horizon, &max_iter, &tol))
    return fail(ctx, -2, "dfm_ss_em: bad arguments");
  DeviceShare gate(ctx->device);
  return ss_em_core(ctx, "dfm_ss_em", X, M, T, N, ldx, stride, spec->dev != 0, starts, n_start, max_iter, tol, spec->update_init != 0,
                    spec->horizon, *out, info);
}

int dfm_ss_em_mf(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                 const dfm_ss_params *starts, int64_t n_start, const dfm_ss_mf *mf, const dfm_ss_em_spec *spec,
                 const dfm_ss_em_out *out, dfm_ss_em_info *info) {
  if (!ctx) return -1;
  if (!mf || N < 1) return fail(ctx, -2, "dfm_ss_em_mf: bad arguments");
  if (!mf->low) return fail(ctx, -2, "dfm_ss_em_mf: the mask of low-frequency series is missing");
  if (!ss_mf_any_low(mf->low, N)) return dfm_ss_em(ctx, X, M, T, N, ldx, stride, starts, n_start, spec, out, info);
  int max_iter = 0;
  double tol = 0.0;
  if (!spec || !out || !starts || n_start < 1 || ss_em_defaults(spec->max_iter, spec->tol, spec->horizon, &max_iter, &tol))
    return fail(ctx, -2, "dfm_ss_em_mf: bad arguments");
  const int r = starts[0].r, p = starts[0].p;
  const int rc = ss_mf_check(r, p, mf->n_w, mf->w, mf->low);
  if (rc == SS_E_LIMIT)
    return fail(ctx, rc, "dfm_ss_em_mf: the mixed-frequency pass serves 1 <= r <= 16, 1 <= p <= 8, 1 <= n_w <= 8, "
                "r max(p, n_w) <= 32");
  if (rc) return fail(ctx, rc, "dfm_ss_em_mf: the weights must be finite with w_0 != 0, and r, p, n_w >= 1");
  const int L = ss_mf_lags(p, mf->n_w);
  std::vector<dfm_ss_params> padded(starts, starts + n_start);
  std::vector<double> Apad((size_t)n_start * r * r * L);
  for (int64_t k = 0; k < n_start; ++k) {
    if (starts[k].r != r || starts[k].p != p || !starts[k].A)
      return fail(ctx, -2, "dfm_ss_em_mf: start %lld has another (r, p)", (long long)k);
    ss_mf_pad_A(starts[k].A, r, p, L, &Apad[(size_t)k * r * r * L]);
    padded[k].p = L;
    padded[k].A = &Apad[(size_t)k * r * r * L];
  }
  DeviceShare gate(ctx->device);
  return ss_em_core(ctx, "dfm_ss_em_mf", X, M, T, N, ldx, stride, spec->dev != 0, padded.data(), n_start, max_iter, tol,
                    spec->update_init != 0, spec->horizon, *out, info, mf, p);
}

int dfm_ss_fit(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
               int horizon, dfm_em_info *info, const dfm_ss_fit_out *out) {
  if (!ctx) return -1;
  return ss_fit_impl(ctx, "dfm_ss_fit", X, T, N, ldx, em_spec, p, horizon, info, out, nullptr, nullptr, nullptr, nullptr);
}

int dfm_ss_fit_ml(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, dfm_em_info *info, const dfm_ss_fit_out *out, double *a0_out,
                  double *loglik_path, dfm_ss_em_info *ml_info) {
  if (!ctx) return -1;
  if (!ml_spec) return fail(ctx, -2, "dfm_ss_fit_ml: bad arguments");
  return ss_fit_impl(ctx, "dfm_ss_fit_ml", X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out, ml_spec, a0_out, loglik_path, ml_info);
}

int dfm_ss_fit_mf(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, const dfm_ss_mf *mf, int method, dfm_em_info *info,
                  const dfm_ss_fit_out *out, double *a0_out, double *loglik_path, dfm_ss_em_info *ml_info,
                  double *smoothed_agg) {
  if (!ctx) return -1;
  if (!ml_spec || !mf || N < 1 || (method != 0 && method != 1)) return fail(ctx, -2, "dfm_ss_fit_mf: bad arguments");
  if (!mf->low) return fail(ctx, -2, "dfm_ss_fit_mf: the mask of low-frequency series is missing");
  if (!ss_mf_any_low(mf->low, N))
    return method ? dfm_ss_fit_ml(ctx, X, T, N, ldx, em_spec, p, ml_spec, info, out, a0_out, loglik_path, ml_info)
                  : dfm_ss_fit(ctx, X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out);
  // r may be selected by the fit: the limits are checked again once it is known
  const int rc = ss_mf_check(em_spec && em_spec->r > 0 ? em_spec->r : 1, p, mf->n_w, mf->w, mf->low);
  if (rc == SS_E_LIMIT)
    return fail(ctx, rc, "dfm_ss_fit_mf: the mixed-frequency pass serves 1 <= r <= 16, 1 <= p <= 8, 1 <= n_w <= 8, "
                "r max(p, n_w) <= 32");
  if (rc) return fail(ctx, rc, "dfm_ss_fit_mf: the weights must be finite with w_0 != 0, and p, n_w >= 1");
  return ss_fit_impl(ctx, "dfm_ss_fit_mf", X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out, method ? ml_spec : nullptr,
                     a0_out, loglik_path, ml_info, mf, smoothed_agg);
}

}  // extern "C"

namespace {

// dfm_ss_fit, and with `ml` dfm_ss_fit_ml: the EM from the two-step parameters
// takes the place of step 5's smoother.
// mf (with a marked series): dfm_ss_fit_mf — the low series' start values by
// ss_mf_start, the padded state, and Lambda ft_t|T for the low columns.
int ss_fit_impl(dfm_ctx *ctx, const char *who, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, const dfm_ss_em_spec *ml, double *a0_out,
                double *loglik_path, dfm_ss_em_info *ml_info, const dfm_ss_mf *mf, double *agg_out) {
  if (!X || !em_spec || !out || T < 2 || N < 1 || ldx < T || horizon < 0)
    return fail(ctx, -2, "%s: bad arguments", who);
  int ml_iter = 0;
  double ml_tol = 0.0;
  if (ml && ss_em_defaults(ml->max_iter, ml->tol, ml->horizon, &ml_iter, &ml_tol))
    return fail(ctx, -2, "%s: bad arguments", who);
  if (p < 1 || p > SS_PMAX) return ss_param_error(ctx, who, p < 1 ? -2 : SS_E_LIMIT, -1);
  const int Lg = mf ? ss_mf_lags(p, mf->n_w) : p;   // lags of the state
  if (em_spec->r > SS_RMAX || (em_spec->r > 0 && em_spec->r * Lg > SS_SMAX))
    return ss_param_error(ctx, who, SS_E_LIMIT, -1);
  DeviceShare gate(ctx->device);
  const size_t tn = (size_t)T * N;
  const int cap = 32;
  std::vector<double> Z(tn), mu((size_t)N), sd((size_t)N), F((size_t)T * cap), L((size_t)N * cap), ev(cap), Xh;
  dfm_em_info inf{};
  int rc = dfm_em(ctx, X, T, N, ldx, em_spec, Z.data(), out->em_completed, mu.data(), sd.data(), F.data(), L.data(),
                  ev.data(), &inf);
  if (rc) return rc;
  const int r = inf.r, s = r * p, sp = r * Lg, h = horizon;   // s: the VAR's columns; sp: the state
  if ((rc = ss_check_dims(r, Lg))) return ss_param_error(ctx, who, rc, -1);
  const double *Xs = X;   // the raw panel on the host: its NaN pattern is the mask
  int64_t lds = ldx;
  if (em_spec->dev) {
    Xh.resize(tn);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpy2DAsync(Xh.data(), (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, (size_t)N,
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    Xs = Xh.data();
    lds = T;
  }
  std::vector<double> Zm(tn);
  for (int64_t i = 0; i < N; ++i)
    for (int64_t t = 0; t < T; ++t)
      Zm[(size_t)i * T + t] = std::isnan(Xs[(size_t)i * lds + t]) ? NAN : Z[(size_t)i * T + t];
  std::vector<double> sig((size_t)N), A((size_t)r * s), Q((size_t)r * r), P0((size_t)s * s);
  int64_t where = -1;
  rc = ss_estimate(Zm.data(), T, N, T, F.data(), L.data(), r, p, sig.data(), A.data(), Q.data(), P0.data(), &where);
  if (rc) return ss_param_error(ctx, who, rc, where);
  const int64_t Tt = T + h;
  std::vector<double> sm((size_t)Tt * r), agg, Apad;
  if (mf) {
    rc = ss_mf_start(Zm.data(), T, N, T, F.data(), r, mf->w, mf->n_w, mf->low, L.data(), sig.data(), &where);
    if (rc == SS_E_VAR)
      return fail(ctx, rc, "%s: low-frequency column %lld (0-based) has fewer than r + 1 observed rows t >= n_w - 1", who,
                  (long long)where);
    if (rc) return ss_param_error(ctx, who, rc, where);
    agg.resize((size_t)Tt * r);
    Apad.resize((size_t)r * sp);
    ss_mf_pad_A(A.data(), r, p, Lg, Apad.data());
    P0.resize((size_t)sp * sp);
    if ((rc = ss_stationary_cov(Apad.data(), Q.data(), r, Lg, P0.data()))) return ss_param_error(ctx, who, rc, -1);
  }
  const double *As = mf ? Apad.data() : A.data();   // the state's A
  if (!ml) {
    const SsParams pr{r, Lg, L.data(), sig.data(), As, Q.data(), nullptr, P0.data()};
    rc = ss_smooth_core(ctx, Zm.data(), 1, T, N, T, (int64_t)tn, false, pr, h, out->filtered, sm.data(),
                        out->smoothed_cov, out->loglik, nullptr, mf, mf ? agg.data() : nullptr);
    if (rc) return rc;
  } else {
    const dfm_ss_params start{r, Lg, L.data(), sig.data(), As, Q.data(), nullptr, P0.data()};
    std::vector<double> L2((size_t)N * r), sig2((size_t)N), A2((size_t)r * s), Q2((size_t)r * r), a02((size_t)sp),
        P02((size_t)sp * sp);
    const dfm_ss_em_out eo{L2.data(), sig2.data(), A2.data(), Q2.data(), a02.data(), P02.data(), out->filtered,
                           sm.data(), out->smoothed_cov, nullptr, loglik_path, mf ? agg.data() : nullptr};
    dfm_ss_em_info mi{};
    rc = ss_em_core(ctx, who, Zm.data(), 1, T, N, T, (int64_t)tn, false, &start, 1, ml_iter, ml_tol, ml->update_init != 0, h,
                    eo, &mi, mf, p);
    if (rc) return rc;
    L = L2, sig = sig2, A = A2, Q = Q2, P0 = P02;
    if (out->loglik) *out->loglik = mi.loglik;
    if (a0_out) std::copy(a02.begin(), a02.end(), a0_out);
    if (ml_info) *ml_info = mi;
  }
  auto put = [](double *dst, const std::vector<double> &v, size_t n) {
    if (dst) std::copy(v.begin(), v.begin() + n, dst);
  };
  put(out->em_standardized, Z, tn);
  put(out->mu, mu, (size_t)N);
  put(out->sd, sd, (size_t)N);
  put(out->em_factors, F, (size_t)T * r);
  put(out->lambda, L, (size_t)N * r);
  put(out->eigvals, ev, (size_t)r);
  put(out->sigma2, sig, (size_t)N);
  put(out->A, A, (size_t)r * s);
  put(out->Q, Q, (size_t)r * r);
  put(out->P0, P0, (size_t)sp * sp);
  put(out->smoothed, sm, (size_t)Tt * r);
  if (mf && agg_out) std::copy(agg.begin(), agg.end(), agg_out);
  // the common component of the smoothed factors, Lambda f_t|T (the fma chain of the EM's); a low-frequency
  // column's is Lambda ft_t|T
  auto common = [&](int64_t t, int64_t i) {
    const double *f = mf && mf->low[i] ? agg.data() : sm.data();
    double c = 0.0;
    for (int j = 0; j < r; ++j) c = fma(f[(size_t)t * r + j], L[(size_t)j * N + i], c);
    return c;
  };
  if (out->x_smoothed || out->x_completed)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t t = 0; t < T; ++t) {
        const double x = Xs[(size_t)i * lds + t];
        const bool obs = !std::isnan(x);
        const double c = obs ? 0.0 : common(t, i);
        if (out->x_smoothed) out->x_smoothed[(size_t)i * T + t] = obs ? Z[(size_t)i * T + t] : c;
        if (out->x_completed) out->x_completed[(size_t)i * T + t] = obs ? x : fma(c, sd[i], mu[i]);
      }
  if (out->forecast)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t k = 0; k < h; ++k) out->forecast[(size_t)i * h + k] = fma(common(T + k, i), sd[i], mu[i]);
  if (info) *info = inf;
  return 0;
}

}  // namespace
