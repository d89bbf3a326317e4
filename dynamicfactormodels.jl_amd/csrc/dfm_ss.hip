// dfm_ss.hip — the state-space pass: a Kalman filter and Rauch-Tung-Striebel
// smoother over the observed entries of M panels of one shape that share the
// parameters (Lambda, sigma^2, A, Q, a0, P0): the E-step of the quasi-ML EM
// (dfm_ss_em.hip) and the last step of the two-step fit (dfm_ss_fit.hip).  The
// model, the recursion and the return codes are stated in include/dfm.h.
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
// For the EM every panel of the batch has its own parameter block (a panel
// stride on the operands, 0 for the shared call) and an `active` flag, and
// ss_smoother_kernel<true> also sums S11, S10, S00 in registers, forms the
// lag-one blocks and writes the M-step GEMM's operand rows.
// The mixed-frequency entry points (dfm_ss_smooth_mf, dfm_ss_em_mf,
// dfm_ss_fit_mf) run the same launches at the padded state: the collapse on
// wider operands (a tri(C) | b group per class), ss_filter_kernel<true>, which
// updates once per class, and ss_smoother_kernel<., true>, which also emits
// Z_l a_t|T and the low class's moments.
// With AR(1) idiosyncratic terms (dfm_ss_smooth_ar, dfm_ss_fit_ar) the state is
// padded to max(p, 2) lags: ss_collapse_ar_kernel forms the quasi-differenced
// pair entries and the start entries from rows t and t - 1 of the panel and
// collapses them to 2r x 2r moments, ss_filter_kernel<false, true> updates at
// that size, and ss_smoother_kernel<false, false> runs unchanged.
//
// The host code states once, for the smoother here and for the EM, the launch
// geometry (ss_geom), a parameter block (ss_block, ss_fill_block), the three
// launches (ss_estep), the messages and the _mf entry points' checks.
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

// The collapse with AR(1) idiosyncratic terms (include/dfm.h): the same tile,
// chunks and output row as ss_collapse_kernel, at the update's size ru = 2r.
// An observed entry whose predecessor is observed is a pair entry, y = x_t -
// rho x_{t-1} against (Wm, Wv); any other observed entry is a start entry, y =
// x_t against (Wsm, Wsv).  The predecessor of a tile's first row is the row
// before it in the panel, that of row 0 is missing.  rho: Npad, zero past N.
// q_t = sum_pair y^2 / sigma^2 + sum_start x^2 (1 - rho^2) / sigma^2.
// A stage is two half-stages through the same four LDS images, the masks with
// their operands and then the values with theirs: the panel is read once and
// the kernel keeps ss_collapse_kernel's 32 KB.
__global__ __launch_bounds__(256) void ss_collapse_ar_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride,
                                                             int T, int N, const double *__restrict__ Wm,
                                                             const double *__restrict__ Wv,
                                                             const double *__restrict__ Wsm,
                                                             const double *__restrict__ Wsv,
                                                             const double *__restrict__ winv,
                                                             const double *__restrict__ rho, int NCP, int nct, int KS,
                                                             int Tpad, int cq, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[4 * 1024];   // two A and two operand images of one half-stage
  double *la0 = lds, *la1 = lds + 1024, *lb0 = lds + 2048, *lb1 = lds + 3072;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int rb = blockIdx.x, cb = blockIdx.y % nct, ks = blockIdx.y / nct, b = blockIdx.z;
  const int abase = rb * 64, bbase = cb * 64;
  const int Npad = (N + 15) & ~15;
  const int k0 = ks * SS_KC, k1 = min(Npad, k0 + SS_KC);
  const bool own_q = cq >= bbase && cq < bbase + 64;
  const double *Xb = X + (int64_t)b * stride;
  const int kk = tid >> 4, g4 = (tid & 15) * 4;
  double acc[8][8];
  tile_zero(acc);
  double qs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int kb = k0; kb < k1; kb += 16) {
    const int n = kb + kk;
    double x[5];   // rows abase + g4 - 1 .. abase + g4 + 3
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int row = abase + g4 + i - 1;
      x[i] = (n < N && row >= 0 && row < T) ? Xb[(int64_t)n * ldx + row] : NAN;
    }
    const int64_t o = (int64_t)n * NCP + bbase + g4;
    const double2 pm0 = *reinterpret_cast<const double2 *>(Wm + o), pm1 = *reinterpret_cast<const double2 *>(Wm + o + 2);
    const double2 sm0 = *reinterpret_cast<const double2 *>(Wsm + o), sm1 = *reinterpret_cast<const double2 *>(Wsm + o + 2);
    const double2 pv0 = *reinterpret_cast<const double2 *>(Wv + o), pv1 = *reinterpret_cast<const double2 *>(Wv + o + 2);
    const double2 sv0 = *reinterpret_cast<const double2 *>(Wsv + o), sv1 = *reinterpret_cast<const double2 *>(Wsv + o + 2);
    const double wi = winv[n], rh = rho[n];
    const double w0 = wi * (1.0 - rh * rh);
    double yp[4], ys[4];   // the pair and the start value of this thread's four rows (0: not of that kind)
    const int ob = ss_offB(g4, kk);
    __syncthreads();   // the previous stage's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool obs = !isnan(x[i + 1]), pair = obs && !isnan(x[i]), start = obs && !pair;
      yp[i] = pair ? fma(-rh, x[i], x[i + 1]) : 0.0;
      ys[i] = start ? x[i + 1] : 0.0;
      la0[ss_offA(g4 + i, kk)] = pair ? 1.0 : 0.0;
      la1[ss_offA(g4 + i, kk)] = start ? 1.0 : 0.0;
      if (own_q) qs[i] = fma(yp[i] * yp[i], wi, fma(ys[i] * ys[i], w0, qs[i]));
    }
    lb0[ob] = pm0.x; lb0[ob + 1] = pm0.y; lb0[ob + 2] = pm1.x; lb0[ob + 3] = pm1.y;
    lb1[ob] = sm0.x; lb1[ob + 1] = sm0.y; lb1[ob + 2] = sm1.x; lb1[ob + 3] = sm1.y;
    __syncthreads();
    tile_step<ss_offA, ss_offB>(acc, la0, lb0, wr, wc, lane);
    tile_step<ss_offA, ss_offB>(acc, la1, lb1, wr, wc, lane);
    __syncthreads();   // the masks' fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      la0[ss_offA(g4 + i, kk)] = yp[i];
      la1[ss_offA(g4 + i, kk)] = ys[i];
    }
    lb0[ob] = pv0.x; lb0[ob + 1] = pv0.y; lb0[ob + 2] = pv1.x; lb0[ob + 3] = pv1.y;
    lb1[ob] = sv0.x; lb1[ob + 1] = sv0.y; lb1[ob + 2] = sv1.x; lb1[ob + 3] = sv1.y;
    __syncthreads();
    tile_step<ss_offA, ss_offB>(acc, la0, lb0, wr, wc, lane);
    tile_step<ss_offA, ss_offB>(acc, la1, lb1, wr, wc, lane);
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
//
// AR: AR(1) idiosyncratic terms (include/dfm.h).  The collapsed row is the
// plain one at ru = 2r, and the update runs on the first ru columns of P and
// entries of a, (f_t, f_{t-1}); r still sizes the companion matrix's dot-product
// rows, Q and the filtered output.  Without AR, ru = r.
template <bool MF, bool AR>
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
  const int ru = AR ? 2 * r : r;   // the size of the update block
  const int nC = ru * (ru + 1) / 2, nG = nC + ru, cq = MF ? 2 * nG : nG, cn = cq + 1, cl = cq + 2;
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
    for (int e = tid; e < ru * ru + ru; e += 256) {
      if (e < ru * ru) {   // G = I + C V beside the identity
        const int i = e / ru, j = e % ru;
        double v = i == j ? 1.0 : 0.0;
        for (int k = 0; k < ru; ++k) v = fma(C(i, k), V[k * SS_LS + j], v);
        GA[i * SS_LS + j] = v;
        GA[i * SS_LS + ru + j] = i == j ? 1.0 : 0.0;
      } else {           // d = b - C z
        const int i = e - ru * ru;
        double v = cr[nC + i];
        for (int k = 0; k < ru; ++k) v = fma(-C(i, k), z[k], v);
        d[i] = v;
      }
    }
    __syncthreads();
    dfm::block_gj_inverse(GA, ru, SS_LS, colj, rowj, sc + 1, &ipiv, &ibad);
    for (int e = tid; e < s * ru + ru; e += 256) {
      if (e < s * ru) {   // K = PZ G^-1
        const int i = e / ru, j = e % ru;
        double v = 0.0;
        for (int k = 0; k < ru; ++k) v = fma(PZ[i * SS_LS + k], GA[k * SS_LS + ru + j], v);
        K[i * SS_LS + j] = v;
      } else {           // G^-1 d
        const int i = e - s * ru;
        double v = 0.0;
        for (int k = 0; k < ru; ++k) v = fma(GA[i * SS_LS + ru + k], d[k], v);
        gv[i] = v;
      }
    }
    __syncthreads();
    for (int e = tid; e < s * ru + s + 1; e += 256) {
      if (e < s * ru) {            // K C
        const int i = e / ru, j = e % ru;
        double v = 0.0;
        for (int k = 0; k < ru; ++k) v = fma(K[i * SS_LS + k], C(k, j), v);
        KC[i * SS_LS + j] = v;
      } else if (e < s * ru + s) {   // a + K d
        const int i = e - s * ru;
        double v = a[i];
        for (int k = 0; k < ru; ++k) v = fma(K[i * SS_LS + k], d[k], v);
        an[i] = v;
      } else {                    // the class's term of the log-likelihood, with z and V from before the update
        double ba = 0.0, aCa = 0.0, dPg = 0.0;
        for (int i = 0; i < ru; ++i) {
          double ca = 0.0, pg = 0.0;
          for (int k = 0; k < ru; ++k) {
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
        for (int k = 0; k < ru; ++k) v = fma(-KC[i * SS_LS + k], PZ[j * SS_LS + k], v);
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
// from the host's memset).  mom: S11, S10, S00, a_1|T, P_1|T at SS_M*
// (dfm_internal.h).
//
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

}  // namespace

int dfm::ss_param_error(dfm_ctx *ctx, const char *who, int rc, int64_t where) {
  switch (rc) {
    case SS_E_LIMIT: return fail(ctx, rc, "%s: the state-space pass serves 1 <= r <= 16, 1 <= p <= 8, r p <= 32", who);
    case SS_E_SIGMA:
      return fail(ctx, rc, "%s: the idiosyncratic variance of column %lld (0-based) is not positive", who, (long long)where);
    case SS_E_VAR: return fail(ctx, rc, "%s: the VAR needs T - p > r p rows and a non-singular Xl'Xl", who);
    case SS_E_NAN: return fail(ctx, rc, "%s: NaN in Lambda, sigma^2, A, Q, a0 or P0", who);
    case SS_E_SINGULAR: return fail(ctx, rc, "%s: Q is not positive definite", who);
    case SS_E_EXPLOSIVE: return fail(ctx, rc, "%s: the VAR is not stationary (the doubling iteration did not converge)", who);
  }
  return fail(ctx, rc, "%s: bad arguments", who);
}

int dfm::ss_ar_error(dfm_ctx *ctx, const char *who, int rc, int64_t where) {
  if (rc == SS_E_LIMIT)
    return fail(ctx, rc, "%s: AR(1) idiosyncratic terms serve 1 <= r <= 8, 1 <= p <= 8, r max(p, 2) <= 32", who);
  if (rc == -2 && where >= 0)
    return fail(ctx, rc, "%s: rho of column %lld (0-based) is not inside (-1, 1)", who, (long long)where);
  if (rc == SS_E_NAN) return fail(ctx, rc, "%s: NaN in rho, F or Lambda", who);
  return ss_param_error(ctx, who, rc, where);
}

int dfm::ss_estep_error(dfm_ctx *ctx, const char *who, long long panel, int flag, int iteration) {
  const char *what = (flag & 2) ? "a G = I + C_t Pff is" : "a P_{t+1|t} is";
  if (iteration < 0) return fail(ctx, SS_E_SINGULAR, "%s: panel %lld: %s not invertible", who, panel, what);
  return fail(ctx, SS_E_SINGULAR, "%s: panel %lld, the E-step of iteration %d: %s not invertible", who, panel, iteration, what);
}

SsGeom dfm::ss_geom(int T, int h, int N, int r, int s, bool mixed, bool ar) {
  SsGeom G;
  G.T = T, G.Tt = T + h, G.N = N, G.r = r, G.s = s, G.mixed = mixed, G.ar = ar, G.ru = ar ? 2 * r : r;
  G.cq = (mixed ? 2 : 1) * (G.ru * (G.ru + 1) / 2 + G.ru), G.ncols = mixed ? G.cq + 4 : ss_ncols(G.ru);
  G.nct = (G.ncols + 63) / 64, G.NCP = G.nct * 64, G.Npad = (N + 15) & ~15;
  G.nrt = (T + 63) / 64, G.Tpad = G.nrt * 64, G.KS = (G.Npad + SS_KC - 1) / SS_KC;
  G.nrn = (N + 63) / 64, G.Nr = G.nrn * 64, G.KT = (((T + 15) & ~15) + SS_KC - 1) / SS_KC;
  return G;
}

// A parameter block: the collapse's operands Wm, Wv (Npad x NCP row-major) and
// winv (Npad), the companion matrix, Q (row-major), a0 (32), P0 (row-major),
// then Lambda (N x r column-major) and sigma^2 (N) as the caller gave them.
// The stride is even: the collapse reads Wm and Wv as double2.
SsBlock dfm::ss_block(const SsGeom &G) {
  const int64_t ss = (int64_t)G.s * G.s;
  SsBlock B;
  const int64_t img = (int64_t)G.Npad * G.NCP;
  B.oWm = 0, B.oWv = B.oWm + img;
  B.oWsm = B.oWv + img, B.oWsv = B.oWsm + (G.ar ? img : 0);   // the start entries' images: AR(1) terms only
  B.owi = B.oWsv + (G.ar ? img : 0);
  B.orho = B.owi + G.Npad;
  B.oTm = B.orho + (G.ar ? G.Npad : 0);
  B.oQ = B.oTm + ss;
  B.oa0 = B.oQ + (int64_t)G.r * G.r;
  B.oP0 = B.oa0 + 32;
  B.oL = B.oP0 + ss;
  B.osig = B.oL + (int64_t)G.N * G.r;
  B.stride = (B.osig + G.N + 1) & ~(int64_t)1;
  return B;
}

// The block of checked parameters; a null P0 is the stationary covariance
// (SS_E_EXPLOSIVE when the doubling iteration does not converge).
// low (mixed frequency): a series' tri(C) | b columns are its class's group
// (the low class's follows the high class's), and the column after l_t counts
// the low class.
// rho (AR(1) terms; G.ar): with z = (lambda, -rho lambda) and z0 = (lambda, 0)
// of size ru, the pair entries' images are tri(z z') / v | 1 | log v and z / v,
// the start entries' those of z0 at the stationary variance v / (1 - rho^2).
int dfm::ss_fill_block(const SsParams &pr, const SsGeom &G, const SsBlock &B, double *hp, const uint8_t *low,
                       const double *rho) {
  const int N = G.N, NCP = G.NCP, r = pr.r, p = pr.p, s = r * p, nC = r * (r + 1) / 2, nG = nC + r, cq = G.cq;
  std::fill(hp, hp + B.stride, 0.0);
  for (int i = 0; i < N && rho; ++i) {
    const double v = pr.sigma2[i], rh = rho[i], c0 = (1.0 - rh * rh) / v;
    const int ru = G.ru, nCu = ru * (ru + 1) / 2;
    double *wm = &hp[B.oWm + (size_t)i * NCP], *wv = &hp[B.oWv + (size_t)i * NCP];
    double *wsm = &hp[B.oWsm + (size_t)i * NCP], *wsv = &hp[B.oWsv + (size_t)i * NCP];
    auto z = [&](int a) { return a < r ? pr.L[(size_t)a * N + i] : -rh * pr.L[(size_t)(a - r) * N + i]; };
    for (int a = 0; a < ru; ++a) {
      for (int c = 0; c <= a; ++c) wm[ss_tri(a, c)] = z(a) * z(c) / v;
      wv[nCu + a] = z(a) / v;
      if (a >= r) continue;
      for (int c = 0; c <= a; ++c) wsm[ss_tri(a, c)] = z(a) * z(c) * c0;
      wsv[nCu + a] = z(a) * c0;
    }
    wm[cq + 1] = wsm[cq + 1] = 1.0;
    wm[cq + 2] = log(v);
    wsm[cq + 2] = log(v / (1.0 - rh * rh));
    hp[B.owi + i] = 1.0 / v;
    hp[B.orho + i] = rh;
  }
  for (int i = 0; i < N && !rho; ++i) {
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

int dfm::ss_estep(dfm_ctx *ctx, const SsGeom &G, const SsBlock &B, const SsEstep &e, int64_t n) {
  hipStream_t st = ctx->stream;
  {
    Scope sc(ctx, DFM_KC_STATS);
    if (G.ar)   // one shared block, every panel active (ss_smooth_core)
      hipLaunchKernelGGL(ss_collapse_ar_kernel, dim3(G.nrt, G.nct * G.KS, (unsigned)n), dim3(256), 0, st, e.X, e.ldx,
                         e.stride, G.T, G.N, e.par + B.oWm, e.par + B.oWv, e.par + B.oWsm, e.par + B.oWsv, e.par + B.owi,
                         e.par + B.orho, G.NCP, G.nct, G.KS, G.Tpad, G.cq, e.part);
    else
      hipLaunchKernelGGL(ss_collapse_kernel, dim3(G.nrt, G.nct * G.KS, (unsigned)n), dim3(256), 0, st, e.X, e.ldx,
                         e.stride, G.T, G.N, e.par + B.oWm, e.par + B.oWv, e.par + B.owi, e.pstride, e.active, G.NCP,
                         G.nct, G.KS, G.Tpad, G.cq, e.part);
  }
  HIPCHK(ctx, hipGetLastError());
  {
    Scope sc(ctx, DFM_KC_MISC);
    SsArgs g{};
    g.T = G.T, g.Tt = G.Tt, g.r = G.r, g.s = G.s, g.ncols = G.ncols, g.KS = G.KS, g.Tpad = G.Tpad, g.NCP = G.NCP;
    g.Tm = e.par + B.oTm, g.Q = e.par + B.oQ, g.a0 = e.par + B.oa0, g.P0 = e.par + B.oP0;
    g.pstride = e.pstride, g.active = e.active, g.part = e.part, g.ws = e.ws;
    g.filt = e.filt, g.smooth = e.smooth, g.cov = e.cov, g.ll = e.ll, g.nobs = e.nobs, g.flag = e.flag;
    g.opnd = e.opnd, g.mom = e.mom, g.nw = e.nw, g.w = e.w, g.agg = e.agg;
    auto *filter = G.ar ? ss_filter_kernel<false, true>
                        : (G.mixed ? ss_filter_kernel<true, false> : ss_filter_kernel<false, false>);
    auto *smoother = e.opnd ? (G.mixed ? ss_smoother_kernel<true, true> : ss_smoother_kernel<true, false>)
                            : (G.mixed ? ss_smoother_kernel<false, true> : ss_smoother_kernel<false, false>);
    hipLaunchKernelGGL(filter, dim3((unsigned)n), dim3(256), 0, st, g);
    hipLaunchKernelGGL(smoother, dim3((unsigned)n), dim3(256), 0, st, g);
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int dfm::ss_mf_args(dfm_ctx *ctx, const char *who, const dfm_ss_mf *mf, int64_t N, bool rest_ok, int r, int p,
                    const char *dims, int *lags) {
  *lags = 0;
  if (!mf || N < 1) return fail(ctx, -2, "%s: bad arguments", who);
  if (!mf->low) return fail(ctx, -2, "%s: the mask of low-frequency series is missing", who);
  if (!ss_mf_any_low(mf->low, N)) return 0;
  if (!rest_ok) return fail(ctx, -2, "%s: bad arguments", who);
  const int rc = ss_mf_check(r, p, mf->n_w, mf->w, mf->low);
  if (rc == SS_E_LIMIT)
    return fail(ctx, rc, "%s: the mixed-frequency pass serves 1 <= r <= 16, 1 <= p <= 8, 1 <= n_w <= 8, "
                "r max(p, n_w) <= 32", who);
  if (rc) return fail(ctx, rc, "%s: the weights must be finite with w_0 != 0, and %s >= 1", who, dims);
  *lags = ss_mf_lags(p, mf->n_w);
  return 0;
}

int64_t dfm::ss_mf_pad_params(const dfm_ss_params *sets, int64_t n, int r, int p, int L, std::vector<dfm_ss_params> &padded,
                              std::vector<double> &Apad) {
  const size_t len = (size_t)r * r * L;
  padded.assign(sets, sets + n);
  Apad.resize((size_t)n * len);
  for (int64_t k = 0; k < n; ++k) {
    if (sets[k].r != r || sets[k].p != p || !sets[k].A) return k;
    ss_mf_pad_A(sets[k].A, r, p, L, &Apad[(size_t)k * len]);
    padded[k].p = L, padded[k].A = &Apad[(size_t)k * len];
  }
  return -1;
}

// The smoother over M panels (layout of dfm_mc).  Outputs host, any nullptr.
// mf: the mixed-frequency model (checked; pr is then the padded state's: p =
// max(p, n_w), A = [A 0]) with its smoothed aggregate agg; null: the plain model.
// after (M = 1): called once the panel's launches are done and checked, with
// what they left on the device (dfm_ss_simulate draws from it); who_plain names
// the plain model's caller in the messages.
int dfm::ss_smooth_core(dfm_ctx *ctx, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx, int64_t stride,
                        bool dev, const SsParams &pr, int h, double *filt, double *smooth, double *cov, double *loglik,
                        int64_t *nobs, const dfm_ss_mf *mf, double *agg, SsAfter *after, const char *who_plain,
                        const double *rho) {
  const char *who = mf ? "dfm_ss_smooth_mf" : who_plain;
  if (rho && (mf || after)) return fail(ctx, -2, "%s: bad arguments", who);
  if (M < 0 || h < 0 || h > (1 << 20)) return fail(ctx, -2, "%s: bad arguments", who);
  int64_t where = -1;
  int rc = ss_check_params(N64, pr.r, pr.p, pr.L, pr.sigma2, pr.A, pr.Q, pr.a0, pr.P0, &where);
  if (rc) return ss_param_error(ctx, who, rc, where);
  if (M == 0) return 0;
  if (!X || T64 < 1 || N64 < 1 || ldx < T64 || stride < ldx * N64) return fail(ctx, -2, "%s: bad panel layout", who);
  if (T64 + h > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "panel too large");
  const SsGeom G = ss_geom((int)T64, h, (int)N64, pr.r, pr.r * pr.p, mf != nullptr, rho != nullptr);
  const int T = G.T, Tt = G.Tt, r = G.r, s = G.s, ss = s * s;
  // ---- the shared parameters: operands of the collapse, companion form, Q, a0, P0, then the weights
  const SsBlock B = ss_block(G);
  const size_t ow = (size_t)B.stride, total = ow + (mf ? SS_WMAX : 0);
  std::vector<double> hp(total);
  if ((rc = ss_fill_block(pr, G, B, hp.data(), mf ? mf->low : nullptr, rho))) return ss_param_error(ctx, who, rc, -1);
  if (mf) std::copy(mf->w, mf->w + mf->n_w, &hp[ow]);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  StreamBuf dpar;
  HIPCHK(ctx, dpar.alloc(total * 8, st));
  double *dp = (double *)dpar.p;
  HIPCHK(ctx, hipMemcpyAsync(dp, hp.data(), total * 8, hipMemcpyHostToDevice, st));
  // ---- panels per pass: the collapsed rows, the recursion's workspace and the outputs
  const size_t per_part = (size_t)G.KS * G.Tpad * G.NCP, per_ws = (size_t)Tt * (2 * (size_t)s + 2 * (size_t)ss),
               per_filt = (size_t)T * r, per_sm = (size_t)Tt * r, per_cov = per_sm * r, per_agg = agg ? per_sm : 0;
  const size_t per = (per_part + per_ws + per_filt + per_sm + per_cov + per_agg + 2) * 8;
  const int64_t mb = ss_panels_per_pass(M, per);
  StreamBuf dwork, dflag;
  SsStage stage{X, ldx, stride, T, G.N, dev, st};
  HIPCHK(ctx, dwork.alloc((size_t)mb * per, st));
  HIPCHK(ctx, dflag.alloc((size_t)mb * 4, st));
  HIPCHK(ctx, stage.alloc(mb));
  double *part = (double *)dwork.p, *ws = part + (size_t)mb * per_part, *dfilt = ws + (size_t)mb * per_ws,
         *dsm = dfilt + (size_t)mb * per_filt, *dcov = dsm + (size_t)mb * per_sm, *dll = dcov + (size_t)mb * per_cov,
         *dn = dll + mb, *dagg = dn + mb;
  SsEstep es{};   // one shared block, every panel active, no moments
  es.ldx = ldx, es.stride = stride, es.par = dp, es.part = part, es.ws = ws;
  es.filt = filt ? dfilt : nullptr, es.smooth = smooth ? dsm : nullptr, es.cov = cov ? dcov : nullptr;
  es.ll = dll, es.nobs = dn, es.flag = (int *)dflag.p;
  es.nw = mf ? mf->n_w : 0, es.w = dp + ow, es.agg = agg ? dagg : nullptr;
  const struct { double *host, *dev; size_t per; } outs[] = {   // what goes back, per panel
      {filt, dfilt, per_filt}, {smooth, dsm, per_sm}, {cov, dcov, per_cov}, {loglik, dll, 1}, {agg, dagg, per_sm}};
  std::vector<int> hflag((size_t)mb);
  std::vector<double> hn((size_t)mb);
  for (int64_t c0 = 0; c0 < M; c0 += mb) {
    const int64_t n = std::min(mb, M - c0);
    HIPCHK(ctx, stage.pass(c0, n, &es.X));
    if ((rc = ss_estep(ctx, G, B, es, n))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(hflag.data(), dflag.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hn.data(), dn, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    for (const auto &o : outs)
      if (o.host) HIPCHK(ctx, hipMemcpyAsync(o.host + c0 * o.per, o.dev, (size_t)n * o.per * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
      if (hflag[i]) return ss_estep_error(ctx, who, c0 + i, hflag[i]);
      if (nobs) nobs[c0 + i] = (int64_t)hn[i];
    }
    if (after && M == 1) {
      const SsKept kept{G, part, ws, dp + B.oTm, dp + B.oP0, &hp[B.oTm], &hp[B.oQ], &hp[B.oa0], &hp[B.oP0]};
      if ((rc = after->run(kept))) return rc;
    }
  }
  return 0;
}

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
  const char *who = "dfm_ss_smooth_mf";
  if (!ctx) return -1;
  if (!params || !spec) return fail(ctx, -2, "%s: bad arguments", who);
  int L = 0;
  if (int rc = ss_mf_args(ctx, who, mf, N, true, params->r, params->p, "r, p, n_w", &L)) return rc;
  if (!L)
    return dfm_ss_smooth(ctx, X, M, T, N, ldx, stride, params, spec, filtered, smoothed, smoothed_cov, loglik, n_observed);
  std::vector<dfm_ss_params> padded;
  std::vector<double> Apad;
  if (ss_mf_pad_params(params, 1, params->r, params->p, L, padded, Apad) >= 0) return fail(ctx, -2, "%s: bad arguments", who);
  const dfm_ss_params &q = padded[0];
  DeviceShare gate(ctx->device);
  const SsParams pr{q.r, q.p, q.lambda, q.sigma2, q.A, q.Q, q.a0, q.P0};
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

int dfm_ss_smooth_ar(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *params, const double *rho, const dfm_ss_spec *spec, double *filtered,
                     double *smoothed, double *smoothed_cov, double *loglik, int64_t *n_observed) {
  const char *who = "dfm_ss_smooth_ar";
  if (!ctx) return -1;
  if (!params || !spec) return fail(ctx, -2, "%s: bad arguments", who);
  int64_t where = -1;
  if (int rc = ss_ar_check(params->r, params->p, N, rho, &where)) return ss_ar_error(ctx, who, rc, where);
  const int L = ss_ar_lags(params->p);
  std::vector<dfm_ss_params> padded;
  std::vector<double> Apad;
  if (ss_mf_pad_params(params, 1, params->r, params->p, L, padded, Apad) >= 0) return fail(ctx, -2, "%s: bad arguments", who);
  const dfm_ss_params &q = padded[0];
  DeviceShare gate(ctx->device);
  const SsParams pr{q.r, q.p, q.lambda, q.sigma2, q.A, q.Q, q.a0, q.P0};
  return ss_smooth_core(ctx, X, M, T, N, ldx, stride, spec->dev != 0, pr, spec->horizon, filtered, smoothed,
                        smoothed_cov, loglik, n_observed, nullptr, nullptr, nullptr, who, rho);
}

int dfm_ss_estimate_ar(dfm_ctx *ctx, const double *Zm, int64_t T, int64_t N, int64_t ldx, const double *F,
                       const double *L, int r, int p, double *sigma_out, double *A_out, double *Q_out, double *P0_out,
                       double *rho_out) {
  if (!ctx) return -1;
  int64_t where = -1;
  const int rc = ss_estimate_ar(Zm, T, N, ldx, F, L, r, p, sigma_out, A_out, Q_out, P0_out, rho_out, &where);
  return rc ? ss_ar_error(ctx, "dfm_ss_estimate_ar", rc, where) : 0;
}

int dfm_ss_ar_fill(const double *X, int64_t T, int64_t N, int64_t ldx, const double *L, int r, const double *rho,
                   const double *smoothed, int64_t horizon, double *completed) {
  if (!X || !L || !smoothed || !completed || T < 1 || ldx < T || horizon < 0 || horizon > (1 << 20)) return -2;
  if (int rc = ss_ar_check(r, 1, N, rho, nullptr)) return rc;
  ss_ar_fill(X, T, N, ldx, L, r, rho, smoothed, horizon, completed);
  return 0;
}

}  // extern "C"
