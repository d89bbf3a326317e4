// dfm_ss_lane.hip — what runs after the smoother's launches for the simulation
// smoother (dfm_ss_sim.hip) and the news decomposition (dfm_ss_news.hip), on
// what ss_smooth_core of dfm_ss.hip hands over:
//   ss_gain_kernel          one workgroup per row t, the rows independent: the
//                           row's K chunks added in the filter's order; per
//                           class (high, low) the flag n^c_t > 0, C^c_t and
//                           K^c_t = PZ G^-1 by the filter's Gauss-Jordan
//                           inverse of G (the low class after the high class's
//                           update of P, recomputed from the stored P_t|t-1),
//                           for the simulation smoother also b_t and the
//                           factor R_t of C_t; then J_t by the smoother's
//                           Cholesky inverse of P_{t+1|t}; into one record per
//                           row (dfm_ss_lane.h)
//   ss_lane_run             the driver: the constants, the gains once, then
//                           per pass the feature's lane kernel and
//   ss_transpose_kernel     the pass's columns from the lanes' layout
//                           [t][k][column] to the caller's [column][t][k]
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_ss_lane.h"

namespace {

struct SsGainArgs {
  int T, Tt, r, s, KS, Tpad, NCP, ncls, nw;
  const double *part, *ws;   // as ss_filter_kernel left them (one panel)
  const double *Tm, *P0;     // s x s row-major
  const double *w;           // ncls = 2: the low class's weights
  double *rec;               // [Tt][ss_rec_len]
};

// Row blockIdx.x.  Matrices in LDS with row stride SS_LS, the products as
// ss_filter_kernel forms them, so K^c_t is the gain the filter applied.  P_t|t-1
// of row 0 is P0 (the filter keeps the predictions of rows >= 1 only).  The
// filter and the smoother have inverted the same matrices by the same steps
// and reported a singular one before this runs: the flag here is not read.
// SIM: the record has room for b_t and R_t.  MF: two classes (g.ncls = 2); as
// in ss_filter_kernel<MF> the collapsed row then needs twice the columns, and
// the plain model's map stays small enough for three workgroups per CU.
template <bool SIM, bool MF>
__global__ __launch_bounds__(256) void ss_gain_kernel(SsGainArgs g) {
  constexpr int NCROW = MF ? 320 : 160;
  __shared__ double lds[6 * SS_MAT + 32 + 64 + NCROW + 4 + (MF ? SS_WMAX : 0)];
  __shared__ int ibad, ipiv;
  double *Tm = lds, *P = Tm + SS_MAT, *W = P + SS_MAT, *GA = W + SS_MAT, *K = GA + SS_MAT, *KC = K + SS_MAT;
  double *colj = KC + SS_MAT, *rowj = colj + 32, *crow = rowj + 64, *sc = crow + NCROW, *wl = sc + 4;
  double *PZl = K + 16, *Vl = KC + 16;   // P Z_l' (s x r) and Z_l P Z_l' (r x r) in the columns K and KC leave free
  const int tid = threadIdx.x, t = blockIdx.x;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s, nw = g.nw;
  constexpr bool mf = MF;
  const int nC = r * (r + 1) / 2, nG = nC + r, cq = mf ? 2 * nG : nG, ncols = cq + (mf ? 4 : 3);
  const int ncl = ss_rec_cls(r, s, SIM);
  const double *Pu = g.ws + (int64_t)Tt * 2 * s, *Pp = Pu + (int64_t)Tt * ss;
  const double *Pprev = t == 0 ? g.P0 : Pp + (int64_t)t * ss;
  double *rec = g.rec + (int64_t)t * ss_rec_len(r, s, g.ncls, SIM);
  double *rJ = rec + ss_rec_fwd(r, s, g.ncls, SIM);
  const int64_t pstep = (int64_t)g.Tpad * g.NCP;
  for (int c = tid; c < ncols; c += 256) {
    double v = 0.0;
    if (t < T)
      for (int k = 0; k < g.KS; ++k) v += g.part[k * pstep + (int64_t)t * g.NCP + c];
    crow[c] = v;
  }
  for (int e = tid; e < ss; e += 256) {
    Tm[(e / s) * SS_LS + e % s] = g.Tm[e];
    P[(e / s) * SS_LS + e % s] = Pprev[e];
  }
  if (mf && tid < nw) wl[tid] = g.w[tid];
  if (tid == 0) ibad = 0;
  __syncthreads();
  const double nt = crow[cq + 1], nl = mf ? crow[cq + 3] : 0.0, nh = nt - nl;
  const bool oh = nt > 0.0 && nh > 0.0, ol = nt > 0.0 && nl > 0.0;
  // One class's gain against Z_c: PZ = P Z_c' (s x r), V = Z_c PZ, the class's
  // moments at column co of the row, its record at rc.  update: P <- P - K C
  // PZ', symmetrised, for the class that follows in this row.
  auto gain = [&](const double *PZ, const double *V, int co, double *rc, bool update) {
    const double *cr = crow + co;
    auto C = [&](int i, int j) { return cr[ss_tri(i, j)]; };
    double *rb = rc + 1, *rC = rc + ss_rec_C(r, SIM), *rR = rC + r * r, *rK = rc + ss_rec_K(r, SIM);
    double *Lw = W;   // SIM: R_t; W is written again only by the update
    for (int e = tid; e < r * r; e += 256) {   // G = I + C V beside the identity
      const int i = e / r, j = e % r;
      double v = i == j ? 1.0 : 0.0;
      for (int k = 0; k < r; ++k) v = fma(C(i, k), V[k * SS_LS + j], v);
      GA[i * SS_LS + j] = v;
      GA[i * SS_LS + r + j] = i == j ? 1.0 : 0.0;
      rC[e] = C(i, j);
      if (SIM) Lw[i * SS_LS + j] = 0.0;
    }
    if (tid == 0) rc[0] = 1.0;
    __syncthreads();
    if (SIM && tid == 0) {   // R_t: the rule of ss_psd_cholesky
      for (int j = 0; j < r; ++j) {
        const double cjj = C(j, j);
        double d = cjj;
        for (int k = 0; k < j; ++k) d -= Lw[j * SS_LS + k] * Lw[j * SS_LS + k];
        if (!(d > 1e-12 * cjj)) continue;
        d = sqrt(d);
        Lw[j * SS_LS + j] = d;
        for (int i = j + 1; i < r; ++i) {
          double v = C(i, j);
          for (int k = 0; k < j; ++k) v -= Lw[i * SS_LS + k] * Lw[j * SS_LS + k];
          Lw[i * SS_LS + j] = v / d;
        }
      }
    }
    dfm::block_gj_inverse(GA, r, SS_LS, colj, rowj, sc + 1, &ipiv, &ibad);
    for (int e = tid; e < s * r; e += 256) {   // K = PZ G^-1
      const int i = e / r, j = e % r;
      double v = 0.0;
      for (int k = 0; k < r; ++k) v = fma(PZ[i * SS_LS + k], GA[k * SS_LS + r + j], v);
      K[i * SS_LS + j] = v;
      rK[e] = v;
    }
    if (SIM)
      for (int e = tid; e < r * r + r; e += 256) {
        if (e < r * r) rR[e] = Lw[(e / r) * SS_LS + e % r];
        else rb[e - r * r] = cr[nC + e - r * r];
      }
    __syncthreads();
    if (!update) return;
    for (int e = tid; e < s * r; e += 256) {   // K C
      const int i = e / r, j = e % r;
      double v = 0.0;
      for (int k = 0; k < r; ++k) v = fma(K[i * SS_LS + k], C(k, j), v);
      KC[i * SS_LS + j] = v;
    }
    __syncthreads();
    for (int e = tid; e < ss; e += 256) {   // P - K C PZ'
      const int i = e / s, j = e % s;
      double v = P[i * SS_LS + j];
      for (int k = 0; k < r; ++k) v = fma(-KC[i * SS_LS + k], PZ[j * SS_LS + k], v);
      W[i * SS_LS + j] = v;
    }
    __syncthreads();
    for (int e = tid; e < ss; e += 256) {
      const int i = e / s, j = e % s;
      P[i * SS_LS + j] = 0.5 * (W[i * SS_LS + j] + W[j * SS_LS + i]);
    }
    __syncthreads();
  };
  if (oh) {
    gain(P, P, 0, rec, ol);
  } else {
    for (int e = tid; e < ncl; e += 256) rec[e] = 0.0;
  }
  if (mf) {
    if (ol) {
      for (int e = tid; e < s * r; e += 256) {   // P Z_l'
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int k = 0; k < nw; ++k) v = fma(wl[k], P[i * SS_LS + k * r + j], v);
        PZl[i * SS_LS + j] = v;
      }
      __syncthreads();
      for (int e = tid; e < r * r; e += 256) {   // Z_l P Z_l'
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int k = 0; k < nw; ++k) v = fma(wl[k], PZl[(k * r + i) * SS_LS + j], v);
        Vl[i * SS_LS + j] = v;
      }
      __syncthreads();
      gain(PZl, Vl, nG, rec + ncl, false);
    } else {
      for (int e = tid; e < ncl; e += 256) rec[ncl + e] = 0.0;
    }
  }
  if (t == Tt - 1) {
    for (int e = tid; e < ss; e += 256) rJ[e] = 0.0;
    return;
  }
  __syncthreads();   // P, GA and K are read
  double *B1 = W, *Lw = GA, *Tw = K;
  for (int e = tid; e < ss; e += 256) {
    P[(e / s) * SS_LS + e % s] = Pu[(int64_t)t * ss + e];
    B1[(e / s) * SS_LS + e % s] = Pp[(int64_t)(t + 1) * ss + e];
  }
  __syncthreads();
  dfm::block_spd_inverse(B1, Lw, Lw, Tw, s, SS_LS, &ibad);   // P_{t+1|t}^-1 into Lw
  for (int e = tid; e < ss; e += 256) {   // P_t|t Tm'
    const int i = e / s, j = e % s;
    double v;
    if (j < r) {
      v = 0.0;
      for (int k = 0; k < s; ++k) v = fma(P[i * SS_LS + k], Tm[j * SS_LS + k], v);
    } else {
      v = P[i * SS_LS + j - r];
    }
    Tw[i * SS_LS + j] = v;
  }
  __syncthreads();
  for (int e = tid; e < ss; e += 256) {   // J = P_t|t Tm' P_{t+1|t}^-1
    const int i = e / s, j = e % s;
    double v = 0.0;
    for (int k = 0; k < s; ++k) v = fma(Tw[i * SS_LS + k], Lw[k * SS_LS + j], v);
    rJ[e] = v;
  }
}

// in: rows x n (the column fastest) -> out: n x rows, by 32 x 32 tiles through LDS;
// tile blockIdx.x % nxt along the columns, blockIdx.x / nxt along the rows.
__global__ __launch_bounds__(256) void ss_transpose_kernel(const double *__restrict__ in, int64_t rows, int64_t n,
                                                           int nxt, double *__restrict__ out) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t x0 = (int64_t)(blockIdx.x % nxt) * 32, y0 = (int64_t)(blockIdx.x / nxt) * 32;
  for (int j = ty; j < 32; j += 8)
    if (x0 + tx < n && y0 + j < rows) tile[j][tx] = in[(y0 + j) * n + x0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (y0 + tx < rows && x0 + j < n) out[(x0 + j) * rows + y0 + tx] = tile[tx][j];
}

hipError_t launch_ss_transpose(const double *in, int64_t rows, int64_t n, double *out, hipStream_t st) {
  const int nxt = (int)((n + 31) / 32);
  const int64_t nyt = (rows + 31) / 32;
  hipLaunchKernelGGL(ss_transpose_kernel, dim3((unsigned)(nxt * nyt)), dim3(256), 0, st, in, rows, n, nxt, out);
  return hipGetLastError();
}

}  // namespace

int dfm::ss_lane_run(dfm_ctx *ctx, const SsKept &k, const SsLaneJob &job, const SsLaneInputs &inputs) {
  const SsGeom &G = k.g;
  const int Tt = G.Tt, r = G.r, s = G.s, ncls = G.mixed ? 2 : 1;
  hipStream_t st = ctx->stream;
  // the simulation smoother has no mixed-frequency model: that gain kernel is not built
  if (job.sim && G.mixed) return fail(ctx, -2, "ss_lane_run: no mixed-frequency record with b_t and R_t");
  StreamBuf dcst, drec, dwork;
  HIPCHK(ctx, dcst.alloc(job.cst.size() * 8, st));
  HIPCHK(ctx, hipMemcpyAsync(dcst.p, job.cst.data(), job.cst.size() * 8, hipMemcpyHostToDevice, st));
  // ---- the gains, once
  HIPCHK(ctx, drec.alloc((size_t)Tt * ss_rec_len(r, s, ncls, job.sim) * 8, st));
  {
    Scope sc(ctx, DFM_KC_OLS);
    const SsGainArgs ga{G.T, Tt, r, s, G.KS, G.Tpad, G.NCP, ncls, job.nw, k.part, k.ws, k.dTm, k.dP0,
                        (const double *)dcst.p + job.w_at, (double *)drec.p};
    auto *gain = job.sim ? ss_gain_kernel<true, false>
                         : (G.mixed ? ss_gain_kernel<false, true> : ss_gain_kernel<false, false>);
    hipLaunchKernelGGL(gain, dim3((unsigned)Tt), dim3(256), 0, st, ga);
  }
  HIPCHK(ctx, hipGetLastError());
  // ---- the columns, in passes: c_t|t, then the planes as the lanes store them and as they leave
  const int64_t np = job.per_pass;
  const size_t per_cf = (size_t)Tt * s, per_out = job.per_out;
  HIPCHK(ctx, dwork.alloc((size_t)np * (per_cf + 2 * job.planes * per_out) * 8, st));
  double *cf = (double *)dwork.p, *o1 = cf + (size_t)np * per_cf, *o2 = o1 + (size_t)np * job.planes * per_out;
  if (job.lds > 65536)   // the attribute is per device: set on every call (cheap)
    HIPCHK(ctx, hipFuncSetAttribute(job.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)job.lds));
  for (int64_t c0 = 0; c0 < job.count; c0 += np) {
    const int64_t n = std::min(np, job.count - c0);
    const SsLaneBufs b{(const double *)dcst.p, (const double *)drec.p, cf, o1, st};
    if (int rc = inputs(c0, n, b)) return rc;   // the pass's own inputs, and job.args for its launch
    {
      Scope sc(ctx, DFM_KC_FACTORS);
      void *args[] = {job.args};
      HIPCHK(ctx, hipLaunchKernel(job.kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), args, job.lds, st));
    }
    const size_t plane = (size_t)n * per_out;   // the pass's planes lie one after the other
    {
      Scope sc(ctx, DFM_KC_GEMM);
      for (int q = 0; q < job.planes; ++q)
        if (job.host[q]) HIPCHK(ctx, launch_ss_transpose(o1 + q * plane, (int64_t)per_out, n, o2 + q * plane, st));
    }
    for (int q = 0; q < job.planes; ++q)
      if (job.host[q])
        HIPCHK(ctx, hipMemcpyAsync(job.host[q] + (size_t)c0 * per_out, o2 + q * plane, plane * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));   // the feature's host staging is reused
  }
  return 0;
}
