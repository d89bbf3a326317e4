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
// No kernel uses an atomic, and the K split depends on N alone: results
// are bit-identical run to run, and panel b of a batch is bit-identical to a
// call on panel b alone.
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_tile.h"

namespace {

constexpr int SS_KC = 256;                    // panel columns per K chunk (a multiple of 16)
constexpr int SS_LS = 33, SS_MAT = 32 * SS_LS;   // row stride and size of an LDS matrix (s <= 32)

DFM_DEV int ss_offA(int a, int kc) { return a * 16 + (kc ^ (((a >> 1) & 1) << 3)); }   // [a][k]
DFM_DEV int ss_offB(int a, int kc) { return kc * 64 + (a ^ ((kc & 7) << 2)); }         // [k][a]

// Columns of a collapsed row: C_t's lower triangle (i (i + 1) / 2 + j), b_t, q_t, n_t, l_t.
__host__ __device__ inline int ss_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
inline int ss_ncols(int r) { return r * (r + 1) / 2 + r + 3; }

// Tile (blockIdx.x, blockIdx.y % nct) of K chunk blockIdx.y / nct of panel
// blockIdx.z.  X: column-major T x N per panel (ldx, stride).  Wm / Wv: the
// operands of the mask and of the values, Npad x NCP row-major, zero past N
// and past ncols; winv: 1 / sigma^2 (Npad, zero past N).  part: [panel][chunk]
// [Tpad][NCP].  q_t = sum x^2 / sigma^2 is summed beside the MFMA by the tile
// that owns its column cq: thread (k, row group) keeps its four rows' sums over
// the stages, and 64 threads add the 16 k in order.
__global__ __launch_bounds__(256) void ss_collapse_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride,
                                                          int T, int N, const double *__restrict__ Wm,
                                                          const double *__restrict__ Wv,
                                                          const double *__restrict__ winv, int NCP, int nct, int KS,
                                                          int Tpad, int cq, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double lds[4 * 1024];   // mask, value, Wm, Wv images of one stage
  double *lm = lds, *lv = lds + 1024, *lbm = lds + 2048, *lbv = lds + 3072;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int rb = blockIdx.x, cb = blockIdx.y % nct, ks = blockIdx.y / nct, b = blockIdx.z;
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
  double *ws;                          // per panel: a_t|t (Tt x s), a_t|t-1 (Tt x s), P_t|t, P_t|t-1 (Tt x s x s each)
  double *filt, *smooth, *cov, *ll, *nobs;   // per panel T x r, Tt x r, Tt x r x r, 1, 1 (nullptr: not wanted)
  int *flag;                           // per panel: 1 a P_{t+1|t} not positive definite, 2 a G singular
};

// Panel blockIdx.x.  Matrices live in LDS with row stride SS_LS; the rows
// i >= r of the companion matrix are the identity shift, so a product with Tm
// or Tm' runs its dot products on the first r rows only and copies the rest.
// P after the update is symmetrised, P after a prediction and the smoothed P
// are computed on the lower triangle and mirrored.  A row without an observed
// entry (n_t = 0; every row t >= T) leaves a and P as they are.  Every
// workspace element is read back by the thread index that wrote it, in the
// filter and (a launch later) in the smoother.
__global__ __launch_bounds__(256) void ss_filter_kernel(SsArgs g) {
  __shared__ double lds[7 * SS_MAT + 7 * 32 + 160 + 4];
  __shared__ int ibad, ipiv;
  double *Tm = lds, *P = Tm + SS_MAT, *W = P + SS_MAT, *GA = W + SS_MAT, *K = GA + SS_MAT, *KC = K + SS_MAT,
         *Qr = KC + SS_MAT;
  double *a = Qr + SS_MAT, *an = a + 32, *d = an + 32, *gv = d + 32, *colj = gv + 32, *rowj = colj + 32,
         *crow = rowj + 64, *sc = crow + 160;   // sc: loglik, log det G, observed count
  const int tid = threadIdx.x, b = blockIdx.x;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s;
  const int cb = r * (r + 1) / 2, cq = cb + r, cn = cq + 1, cl = cq + 2;
  double *au = g.ws + (int64_t)b * Tt * (2 * s + 2 * ss), *ap = au + (int64_t)Tt * s, *Pu = ap + (int64_t)Tt * s,
         *Pp = Pu + (int64_t)Tt * ss;
  const double *part = g.part + (int64_t)b * g.KS * (int64_t)g.Tpad * g.NCP;
  const int64_t pstep = (int64_t)g.Tpad * g.NCP;
  for (int e = tid; e < ss; e += 256) {
    const int i = e / s, j = e % s;
    Tm[i * SS_LS + j] = g.Tm[e];
    P[i * SS_LS + j] = g.P0[e];
  }
  for (int e = tid; e < r * r; e += 256) Qr[(e / r) * SS_LS + e % r] = g.Q[e];
  if (tid < s) a[tid] = g.a0[tid];
  if (tid < 3) sc[tid] = 0.0;
  if (tid == 0) ibad = 0;
  __syncthreads();
  auto C = [&](int i, int j) { return crow[ss_tri(i, j)]; };
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
    if (nt > 0.0) {
      for (int e = tid; e < r * r + r; e += 256) {
        if (e < r * r) {   // G = I + C Pff beside the identity
          const int i = e / r, j = e % r;
          double v = i == j ? 1.0 : 0.0;
          for (int k = 0; k < r; ++k) v = fma(C(i, k), P[k * SS_LS + j], v);
          GA[i * SS_LS + j] = v;
          GA[i * SS_LS + r + j] = i == j ? 1.0 : 0.0;
        } else {           // d = b - C a_f
          const int i = e - r * r;
          double v = crow[cb + i];
          for (int k = 0; k < r; ++k) v = fma(-C(i, k), a[k], v);
          d[i] = v;
        }
      }
      __syncthreads();
      dfm::block_gj_inverse(GA, r, SS_LS, colj, rowj, sc + 1, &ipiv, &ibad);
      for (int e = tid; e < s * r + r; e += 256) {
        if (e < s * r) {   // K = Pf G^-1
          const int i = e / r, j = e % r;
          double v = 0.0;
          for (int k = 0; k < r; ++k) v = fma(P[i * SS_LS + k], GA[k * SS_LS + r + j], v);
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
        } else {                    // the row's term of the log-likelihood, with a_f and Pff from before the update
          double ba = 0.0, aCa = 0.0, dPg = 0.0;
          for (int i = 0; i < r; ++i) {
            double ca = 0.0, pg = 0.0;
            for (int k = 0; k < r; ++k) {
              ca = fma(C(i, k), a[k], ca);
              pg = fma(P[i * SS_LS + k], gv[k], pg);
            }
            ba = fma(crow[cb + i], a[i], ba);
            aCa = fma(a[i], ca, aCa);
            dPg = fma(d[i], pg, dPg);
          }
          sc[0] -= 0.5 * (nt * 1.8378770664093453 + crow[cl] + sc[1] + crow[cq] - 2.0 * ba + aCa - dPg);
          sc[2] += nt;
        }
      }
      __syncthreads();
      for (int e = tid; e < ss + s; e += 256) {
        if (e < ss) {   // P - K C Pf'
          const int i = e / s, j = e % s;
          double v = P[i * SS_LS + j];
          for (int k = 0; k < r; ++k) v = fma(-KC[i * SS_LS + k], P[j * SS_LS + k], v);
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
__global__ __launch_bounds__(256) void ss_smoother_kernel(SsArgs g) {
  __shared__ double lds[7 * SS_MAT + 4 * 32];
  __shared__ int ibad;
  double *Tm = lds, *P = Tm + SS_MAT, *B1 = P + SS_MAT, *Lw = B1 + SS_MAT, *Tw = Lw + SS_MAT, *J = Tw + SS_MAT,
         *Ps = J + SS_MAT;
  double *a = Ps + SS_MAT, *an = a + 32, *d = an + 32, *gv = d + 32;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Tt = g.Tt, r = g.r, s = g.s, ss = s * s;
  const double *au = g.ws + (int64_t)b * Tt * (2 * s + 2 * ss), *ap = au + (int64_t)Tt * s,
               *Pu = ap + (int64_t)Tt * s, *Pp = Pu + (int64_t)Tt * ss;
  auto emit = [&](int t) {   // a and Ps hold row t's smoothed moments
    if (g.smooth && tid < r) g.smooth[((int64_t)b * Tt + t) * r + tid] = a[tid];
    if (g.cov)
      for (int e = tid; e < r * r; e += 256) g.cov[((int64_t)b * Tt + t) * r * r + e] = Ps[(e / r) * SS_LS + e % r];
  };
  for (int e = tid; e < ss; e += 256) {
    Tm[(e / s) * SS_LS + e % s] = g.Tm[e];
    Ps[(e / s) * SS_LS + e % s] = Pu[(int64_t)(Tt - 1) * ss + e];
  }
  if (tid < s) a[tid] = au[(int64_t)(Tt - 1) * s + tid];
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
  }
  if (tid == 0 && ibad) g.flag[b] |= 1;
}

// One device block, freed on the stream on every return path.
struct StreamBuf {
  void *p = nullptr;
  hipStream_t st = nullptr;
  ~StreamBuf() {
    if (p) hipFreeAsync(p, st);
  }
  hipError_t alloc(size_t bytes, hipStream_t s) {
    st = s;
    return stream_malloc(&p, std::max<size_t>(bytes, 8), s);
  }
};

struct SsParams {   // checked, host
  int r = 0, p = 0;
  const double *L = nullptr, *sigma2 = nullptr, *A = nullptr, *Q = nullptr, *a0 = nullptr, *P0 = nullptr;
};

int ss_param_error(dfm_ctx *ctx, const char *who, int rc, int64_t where) {
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

// The smoother over M panels (layout of dfm_mc).  Outputs host, any nullptr.
int ss_smooth_core(dfm_ctx *ctx, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx, int64_t stride,
                   bool dev, const SsParams &pr, int h, double *filt, double *smooth, double *cov, double *loglik,
                   int64_t *nobs) {
  if (M < 0 || h < 0 || h > (1 << 20)) return fail(ctx, -2, "dfm_ss_smooth: bad arguments");
  int64_t where = -1;
  int rc = ss_check_params(N64, pr.r, pr.p, pr.L, pr.sigma2, pr.A, pr.Q, pr.a0, pr.P0, &where);
  if (rc) return ss_param_error(ctx, "dfm_ss_smooth", rc, where);
  if (M == 0) return 0;
  if (!X || T64 < 1 || N64 < 1 || ldx < T64 || stride < ldx * N64) return fail(ctx, -2, "dfm_ss_smooth: bad panel layout");
  if (T64 + h > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "panel too large");
  const int T = (int)T64, N = (int)N64, r = pr.r, p = pr.p, s = r * p, ss = s * s, Tt = T + h;
  const int ncols = ss_ncols(r), nct = (ncols + 63) / 64, NCP = nct * 64, Npad = (N + 15) & ~15;
  const int nrt = (T + 63) / 64, Tpad = nrt * 64, KS = (Npad + SS_KC - 1) / SS_KC;
  const int nC = r * (r + 1) / 2, cq = nC + r;
  // ---- the shared parameters: operands of the collapse, companion form, Q, a0, P0
  std::vector<double> hp;
  const size_t oWm = 0, oWv = oWm + (size_t)Npad * NCP, owi = oWv + (size_t)Npad * NCP, oTm = owi + Npad,
               oQ = oTm + ss, oa0 = oQ + (size_t)r * r, oP0 = oa0 + 32, total = oP0 + ss;
  hp.assign(total, 0.0);
  for (int i = 0; i < N; ++i) {
    const double v = pr.sigma2[i];
    double *wm = &hp[oWm + (size_t)i * NCP], *wv = &hp[oWv + (size_t)i * NCP];
    for (int a = 0; a < r; ++a) {
      const double la = pr.L[(size_t)a * N + i];
      for (int c = 0; c <= a; ++c) wm[ss_tri(a, c)] = la * pr.L[(size_t)c * N + i] / v;
      wv[nC + a] = la / v;
    }
    wm[cq + 1] = 1.0;
    wm[cq + 2] = log(v);
    hp[owi + i] = 1.0 / v;
  }
  ss_companion(pr.A, r, p, &hp[oTm]);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) hp[oQ + i * r + j] = pr.Q[(size_t)j * r + i];
  if (pr.a0) std::copy(pr.a0, pr.a0 + s, &hp[oa0]);
  if (pr.P0) {
    for (int i = 0; i < s; ++i)
      for (int j = 0; j < s; ++j) hp[oP0 + i * s + j] = pr.P0[(size_t)j * s + i];
  } else if ((rc = ss_stationary_cov(pr.A, pr.Q, r, p, &hp[oP0]))) {
    return ss_param_error(ctx, "dfm_ss_smooth", rc, -1);
  }
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  StreamBuf dpar;
  HIPCHK(ctx, dpar.alloc(total * 8, st));
  double *dp = (double *)dpar.p;
  HIPCHK(ctx, hipMemcpyAsync(dp, hp.data(), total * 8, hipMemcpyHostToDevice, st));
  // ---- panels per pass: the collapsed rows and the recursion's workspace, about half a GB at the most
  const size_t per_part = (size_t)KS * Tpad * NCP, per_ws = (size_t)Tt * (2 * (size_t)s + 2 * (size_t)ss),
               per_out = (size_t)T * r + (size_t)Tt * r + (size_t)Tt * r * r + 2;
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
         *dcov = dsm + (size_t)mb * Tt * r, *dll = dcov + (size_t)mb * Tt * r * r, *dn = dll + mb;
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
                         dp + oWm, dp + oWv, dp + owi, NCP, nct, KS, Tpad, cq, part);
    }
    HIPCHK(ctx, hipGetLastError());
    {
      Scope sc(ctx, DFM_KC_MISC);
      SsArgs g{T, Tt, r, s, ncols, KS, Tpad, NCP, part, dp + oTm, dp + oQ, dp + oa0, dp + oP0, ws,
               filt ? dfilt : nullptr, smooth ? dsm : nullptr, cov ? dcov : nullptr, dll, dn, (int *)dflag.p};
      hipLaunchKernelGGL(ss_filter_kernel, dim3((unsigned)n), dim3(256), 0, st, g);
      hipLaunchKernelGGL(ss_smoother_kernel, dim3((unsigned)n), dim3(256), 0, st, g);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(hflag.data(), dflag.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hn.data(), dn, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (filt) HIPCHK(ctx, hipMemcpyAsync(filt + c0 * T * r, dfilt, (size_t)n * T * r * 8, hipMemcpyDeviceToHost, st));
    if (smooth) HIPCHK(ctx, hipMemcpyAsync(smooth + c0 * Tt * r, dsm, (size_t)n * Tt * r * 8, hipMemcpyDeviceToHost, st));
    if (cov)
      HIPCHK(ctx, hipMemcpyAsync(cov + c0 * Tt * r * r, dcov, (size_t)n * Tt * r * r * 8, hipMemcpyDeviceToHost, st));
    if (loglik) HIPCHK(ctx, hipMemcpyAsync(loglik + c0, dll, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i < n; ++i) {
      if (hflag[i])
        return fail(ctx, SS_E_SINGULAR, "dfm_ss_smooth: panel %lld: %s not invertible", (long long)(c0 + i),
                    (hflag[i] & 2) ? "a G = I + C_t Pff is" : "a P_{t+1|t} is");
      if (nobs) nobs[c0 + i] = (int64_t)hn[i];
    }
  }
  return 0;
}

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

int dfm_ss_estimate(dfm_ctx *ctx, const double *Zm, int64_t T, int64_t N, int64_t ldx, const double *F, const double *L,
                    int r, int p, double *sigma_out, double *A_out, double *Q_out, double *P0_out) {
  if (!ctx) return -1;
  int64_t where = -1;
  const int rc = ss_estimate(Zm, T, N, ldx, F, L, r, p, sigma_out, A_out, Q_out, P0_out, &where);
  return rc ? ss_param_error(ctx, "dfm_ss_estimate", rc, where) : 0;
}

int dfm_ss_fit(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
               int horizon, dfm_em_info *info, const dfm_ss_fit_out *out) {
  if (!ctx) return -1;
  if (!X || !em_spec || !out || T < 2 || N < 1 || ldx < T || horizon < 0)
    return fail(ctx, -2, "dfm_ss_fit: bad arguments");
  if (p < 1 || p > SS_PMAX) return ss_param_error(ctx, "dfm_ss_fit", p < 1 ? -2 : SS_E_LIMIT, -1);
  if (em_spec->r > SS_RMAX || (em_spec->r > 0 && em_spec->r * p > SS_SMAX))
    return ss_param_error(ctx, "dfm_ss_fit", SS_E_LIMIT, -1);
  DeviceShare gate(ctx->device);
  const size_t tn = (size_t)T * N;
  const int cap = 32;
  std::vector<double> Z(tn), mu((size_t)N), sd((size_t)N), F((size_t)T * cap), L((size_t)N * cap), ev(cap), Xh;
  dfm_em_info inf{};
  int rc = dfm_em(ctx, X, T, N, ldx, em_spec, Z.data(), out->em_completed, mu.data(), sd.data(), F.data(), L.data(),
                  ev.data(), &inf);
  if (rc) return rc;
  const int r = inf.r, s = r * p, h = horizon;
  if ((rc = ss_check_dims(r, p))) return ss_param_error(ctx, "dfm_ss_fit", rc, -1);
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
  if (rc) return ss_param_error(ctx, "dfm_ss_fit", rc, where);
  const int64_t Tt = T + h;
  std::vector<double> sm((size_t)Tt * r);
  const SsParams pr{r, p, L.data(), sig.data(), A.data(), Q.data(), nullptr, P0.data()};
  rc = ss_smooth_core(ctx, Zm.data(), 1, T, N, T, (int64_t)tn, false, pr, h, out->filtered, sm.data(), out->smoothed_cov,
                      out->loglik, nullptr);
  if (rc) return rc;
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
  put(out->P0, P0, (size_t)s * s);
  put(out->smoothed, sm, (size_t)Tt * r);
  // the common component of the smoothed factors, Lambda f_t|T (the fma chain of the EM's)
  auto common = [&](int64_t t, int64_t i) {
    double c = 0.0;
    for (int j = 0; j < r; ++j) c = fma(sm[(size_t)t * r + j], L[(size_t)j * N + i], c);
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

}  // extern "C"
