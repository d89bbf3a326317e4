// dfm_ss_news.hip — the news decomposition of Banbura & Modugno (2014) on top
// of the state-space pass: which release moved the smoothed path between two
// vintages of one panel, and by how much (dfm_ss_news; the mathematics, the
// layouts and the return codes are stated in include/dfm.h).
//
// The smoother's own launches run on X_old, X_rev and X_new (ss_smooth_core of
// dfm_ss.hip); the last run hands over what it leaves on the device, then
//   ss_news_gain_kernel   one workgroup per row t, the rows independent: per
//                         class (high, low) the flag n^c_t > 0, C^c_t and K^c_t
//                         = PZ G^-1 by the filter's steps (the low class after
//                         the high class's update of P, recomputed from the
//                         stored P_t|t-1), then J_t by the smoother's steps,
//                         into one record per row
//   ss_news_kernel        one lane per release, one wave per workgroup: the
//                         impulse response c forwards from the lane's own row
//                         t_j, c_t|T backwards down to t_lo; a lane's state
//                         lives in LDS columns [k][lane], the row's record is
//                         staged in LDS once per wave and read by broadcast
// and the transposing kernel of dfm_ss_sim.hip brings the pass's weights from
// the lanes' layout [t][k][release] to the caller's [release][t][k].
// No lane reads another lane's values: a release's weights depend on neither
// J, its lane nor its pass.
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_ss_lane.h"

namespace {

// A row's record: per class c < ncls the flag n^c_t > 0 (1.0 / 0.0), C^c_t
// (r x r) and K^c_t (s x r) — what the forward pass reads — then J_t (s x s),
// all row-major.
__host__ __device__ inline int news_rec_cls(int r, int s) { return 1 + r * r + s * r; }
__host__ __device__ inline int news_rec_fwd(int r, int s, int ncls) { return ncls * news_rec_cls(r, s); }
__host__ __device__ inline int news_rec_len(int r, int s, int ncls) { return news_rec_fwd(r, s, ncls) + s * s; }

struct NewsGainArgs {
  int T, Tt, r, s, KS, Tpad, NCP, ncls, nw;
  const double *part, *ws;   // as the filter left them (one panel)
  const double *Tm, *P0;     // s x s row-major
  const double *w;           // ncls = 2: the low class's weights
  double *rec;               // [Tt][news_rec_len]
};

// Row blockIdx.x.  Matrices in LDS with row stride SS_LS, the products as
// ss_filter_kernel forms them, so K^c_t is the gain the filter applied.  P_t|t-1
// of row 0 is P0.  The filter and the smoother have inverted the same matrices
// by the same steps and reported a singular one before this runs: the flag
// here is not read.
__global__ __launch_bounds__(256) void ss_news_gain_kernel(NewsGainArgs g) {
  __shared__ double lds[6 * SS_MAT + 32 + 64 + 320 + 4 + SS_WMAX];
  __shared__ int ibad, ipiv;
  double *Tm = lds, *P = Tm + SS_MAT, *W = P + SS_MAT, *GA = W + SS_MAT, *K = GA + SS_MAT, *KC = K + SS_MAT;
  double *colj = KC + SS_MAT, *rowj = colj + 32, *crow = rowj + 64, *sc = crow + 320, *wl = sc + 4;
  double *PZl = K + 16, *Vl = KC + 16;   // P Z_l' (s x r) and Z_l P Z_l' (r x r) in the columns K and KC leave free
  const int tid = threadIdx.x, t = blockIdx.x;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s, nw = g.nw;
  const bool mf = g.ncls == 2;
  const int nC = r * (r + 1) / 2, nG = nC + r, cq = mf ? 2 * nG : nG, ncols = cq + (mf ? 4 : 3);
  const int ncl = news_rec_cls(r, s);
  const double *Pu = g.ws + (int64_t)Tt * 2 * s, *Pp = Pu + (int64_t)Tt * ss;
  const double *Pprev = t == 0 ? g.P0 : Pp + (int64_t)t * ss;
  double *rec = g.rec + (int64_t)t * news_rec_len(r, s, g.ncls);
  double *rJ = rec + news_rec_fwd(r, s, g.ncls);
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
    double *rC = rc + 1, *rK = rC + r * r;
    for (int e = tid; e < r * r; e += 256) {   // G = I + C V beside the identity
      const int i = e / r, j = e % r;
      double v = i == j ? 1.0 : 0.0;
      for (int k = 0; k < r; ++k) v = fma(C(i, k), V[k * SS_LS + j], v);
      GA[i * SS_LS + j] = v;
      GA[i * SS_LS + r + j] = i == j ? 1.0 : 0.0;
      rC[e] = C(i, j);
    }
    if (tid == 0) rc[0] = 1.0;
    __syncthreads();
    dfm::block_gj_inverse(GA, r, SS_LS, colj, rowj, sc + 1, &ipiv, &ibad);
    for (int e = tid; e < s * r; e += 256) {   // K = PZ G^-1
      const int i = e / r, j = e % r;
      double v = 0.0;
      for (int k = 0; k < r; ++k) v = fma(PZ[i * SS_LS + k], GA[k * SS_LS + r + j], v);
      K[i * SS_LS + j] = v;
      rK[e] = v;
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

struct NewsArgs {
  int Tt, t_lo, r, s, n, nw;   // n: the pass's releases
  const int *row;              // the pass's releases: t_j (n), then the class c(i_j) (n)
  const double *beta;          // lambda_{i_j} / sigma^2_{i_j}: entry k of release d at beta[k n + d]
  const double *rec;           // ss_news_gain_kernel's records
  const double *cst;           // the companion matrix's first r rows (r x s row-major), then the weights (SS_WMAX)
  double *cf;                  // c_t|t [Tt][s][n]
  double *wf, *wa;             // c_t|T[:r] and Z_l c_t|T, [Tt - t_lo][r][n] each (wa: MF only)
};

// 64 PRE >= the forward record and J_t at r = 16, s = 32
template <bool MF> constexpr int NEWS_PRE = MF ? 25 : 16;

// LDS doubles of ss_news_kernel: the companion rows, the weights, one staged
// record, and the columns of c (s), c_t|t (s), the work vector (max(s, 2 r))
// and beta (r).
inline size_t ss_news_lds(int r, int s, int ncls) {
  return (size_t)(r * s + SS_WMAX + std::max(news_rec_fwd(r, s, ncls), s * s) + (2 * s + std::max(s, 2 * r) + r) * 64);
}

// Release blockIdx.x * 64 + lane of the pass.  The layout and the staging are
// ss_sim_kernel's: element k of a lane's vector at [k * 64 + lane], the next
// row's record fetched into registers while this row is computed, two barriers
// per row around the staging buffer (the workgroup is one wave).  The releases
// are sorted by row, so the wave's forward loop starts at its first lane's t_j;
// a lane does nothing before its own row (its c is zero there), and neither
// loop contains a barrier inside a lane's condition.  A lane past the pass's
// last release never starts and stores nothing.
template <bool MF>
__global__ __launch_bounds__(64) void ss_news_kernel(NewsArgs g) {
  extern __shared__ __attribute__((aligned(16))) double news_lds[];
  constexpr int NCLS = MF ? 2 : 1, PRE = NEWS_PRE<MF>;
  const int Tt = g.Tt, t_lo = g.t_lo, r = g.r, s = g.s, n = g.n, nw = g.nw, lane = threadIdx.x;
  const int ncl = news_rec_cls(r, s), nf = NCLS * ncl, nrec = nf + s * s, ss = s * s;
  double *Tmr = news_lds, *wl = Tmr + r * s, *st = wl + SS_WMAX;
  double *Cc = st + (nf > ss ? nf : ss) + lane, *A = Cc + s * 64, *W = A + s * 64;   // this lane's columns
  double *B = W + (s > 2 * r ? s : 2 * r) * 64;
  const int64_t d = (int64_t)blockIdx.x * 64 + lane;
  const bool act = d < n;
  const int tj = act ? g.row[d] : Tt, cj = act ? g.row[n + d] : 0;
  const int t0 = g.row[(int64_t)blockIdx.x * 64];   // the wave's smallest row
  for (int e = lane; e < r * s + SS_WMAX; e += 64) Tmr[e] = g.cst[e];   // Tmr and wl are adjacent on both sides
  double pre[PRE];
  auto fetch = [&](const double *src, int len) {
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = lane + 64 * q;
      pre[q] = e < len ? src[e] : 0.0;
    }
  };
  auto stage = [&](int len) {
    __syncthreads();   // the previous record is read
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = lane + 64 * q;
      if (e < len) st[e] = pre[q];
    }
    __syncthreads();
  };
  double lp[32];   // the lane's own next row of c_t|t
  auto lfetch = [&](int t) {
    const bool have = act && t >= t0;   // c_t|t of a row before the wave's first is zero and was not stored
#pragma unroll
    for (int q = 0; q < 32; ++q) lp[q] = (have && q < s) ? g.cf[((int64_t)t * s + q) * n + d] : 0.0;
  };
  auto lput = [&](double *x) {
#pragma unroll
    for (int q = 0; q < 32; ++q)
      if (q < s) x[q * 64] = lp[q];
  };
  // x <- Tm x on a lane's column: the first r rows by dot products into W, the rest a shift
  auto advance = [&](double *x) {
    for (int i = 0; i < r; ++i) W[i * 64] = sim_dot<false>(0.0, Tmr + i * s, x, s);
    for (int i = s - 1; i >= r; --i) x[i * 64] = x[(i - r) * 64];
    for (int i = 0; i < r; ++i) x[i * 64] = W[i * 64];
  };
  // Z_l x of a lane's column into y
  auto aggregate = [&](const double *x, double *y) {
    for (int i = 0; i < r; ++i) {
      double v = 0.0;
      for (int k = 0; k < nw; ++k) v = fma(wl[k], x[(k * r + i) * 64], v);
      y[i * 64] = v;
    }
  };
  auto emit = [&](int t) {   // Cc holds c_t|T
    if (!act) return;
    const int64_t o = (int64_t)(t - t_lo) * r;
    for (int i = 0; i < r; ++i) g.wf[(o + i) * n + d] = Cc[i * 64];
    if (MF) {
      aggregate(Cc, W);
      for (int i = 0; i < r; ++i) g.wa[(o + i) * n + d] = W[i * 64];
    }
  };
  for (int i = 0; i < s; ++i) Cc[i * 64] = 0.0;
  for (int i = 0; i < r; ++i) B[i * 64] = act ? g.beta[(int64_t)i * n + d] : 0.0;
  fetch(g.rec + (int64_t)t0 * nrec, nf);
  // ---------------------------------------------------------------- forwards
  for (int t = t0; t < Tt; ++t) {
    stage(nf);
    if (t + 1 < Tt) fetch(g.rec + (int64_t)(t + 1) * nrec, nf);
    else if (Tt >= 2) fetch(g.rec + (int64_t)(Tt - 2) * nrec + nf, ss);
    const bool on = t >= tj;
    if (on) {
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        const double *rc = st + c * ncl;
        if (rc[0] == 0.0) continue;
        const double *C = rc + 1, *K = C + r * r;
        const double *z = Cc;
        if (c == 1) {
          aggregate(Cc, W + r * 64);
          z = W + r * 64;
        }
        const bool hit = t == tj && c == cj;
        for (int i = 0; i < r; ++i) W[i * 64] = sim_dot<true>(hit ? B[i * 64] : 0.0, C + i * r, z, r);   // d = beta - C z
        for (int i = 0; i < s; ++i) Cc[i * 64] = sim_dot<false>(Cc[i * 64], K + i * r, W, r);
      }
    }
    if (t == Tt - 1) break;
    if (act)
      for (int i = 0; i < s; ++i) g.cf[((int64_t)t * s + i) * n + d] = Cc[i * 64];
    if (on) advance(Cc);
  }
  // --------------------------------------------------------------- backwards
  emit(Tt - 1);
  if (Tt - 2 >= t_lo) lfetch(Tt - 2);
  for (int t = Tt - 2; t >= t_lo; --t) {
    stage(ss);   // J_t
    lput(A);     // c_t|t
    if (t - 1 >= t_lo) {
      fetch(g.rec + (int64_t)(t - 1) * nrec + nf, ss);
      lfetch(t - 1);
    }
    for (int i = 0; i < s; ++i) {   // c_{t+1|T} - Tm c_t|t
      const double v = i < r ? sim_dot<false>(0.0, Tmr + i * s, A, s) : A[(i - r) * 64];
      W[i * 64] = Cc[i * 64] - v;
    }
    for (int i = 0; i < s; ++i) Cc[i * 64] = sim_dot<false>(A[i * 64], st + i * s, W, s);
    emit(t);
  }
}

// The weights of every release, from what the smoother's launches on X_new
// left on the device.
struct NewsRun : SsAfter {
  dfm_ctx *ctx = nullptr;
  int64_t J = 0, pass_releases = 0;
  int t_lo = 0;
  const int64_t *rel_t = nullptr, *rel_i = nullptr;
  const double *L = nullptr, *sigma2 = nullptr;   // N x r column-major, N
  const uint8_t *low = nullptr;                   // null: the plain model
  const double *w = nullptr;
  int nw = 0;
  double *wf = nullptr, *wa = nullptr;            // host, J x (Tt - t_lo) x r; either may be null

  int run(const SsKept &k) override {
    const SsGeom &G = k.g;
    const int Tt = G.Tt, r = G.r, s = G.s, ncls = G.mixed ? 2 : 1, nrec = news_rec_len(r, s, ncls);
    hipStream_t st = ctx->stream;
    // ---- the constants: the companion matrix's first r rows, the weights
    std::vector<double> hc((size_t)r * s + SS_WMAX, 0.0);
    std::copy(k.hTm, k.hTm + r * s, hc.begin());
    if (G.mixed) std::copy(w, w + nw, &hc[(size_t)r * s]);
    StreamBuf dcst, drec, dwork, drow;
    HIPCHK(ctx, dcst.alloc(hc.size() * 8, st));
    HIPCHK(ctx, hipMemcpyAsync(dcst.p, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, st));
    // ---- the gains, once
    HIPCHK(ctx, drec.alloc((size_t)Tt * nrec * 8, st));
    {
      Scope sc(ctx, DFM_KC_OLS);
      const NewsGainArgs ga{G.T, Tt, r, s, G.KS, G.Tpad, G.NCP, ncls, nw, k.part, k.ws, k.dTm, k.dP0,
                            (const double *)dcst.p + r * s, (double *)drec.p};
      hipLaunchKernelGGL(ss_news_gain_kernel, dim3((unsigned)Tt), dim3(256), 0, st, ga);
    }
    HIPCHK(ctx, hipGetLastError());
    // ---- the releases, in passes
    const bool agg = G.mixed && wa;
    const int64_t np = ss_news_releases_per_pass(Tt, t_lo, r, s, G.mixed, J, pass_releases);
    const size_t per_cf = (size_t)Tt * s, per_out = (size_t)(Tt - t_lo) * r, nout = G.mixed ? 2 : 1;
    HIPCHK(ctx, dwork.alloc((size_t)np * (per_cf + 2 * nout * per_out + r) * 8, st));
    HIPCHK(ctx, drow.alloc((size_t)np * 2 * 4, st));
    double *cf = (double *)dwork.p, *o1 = cf + (size_t)np * per_cf, *o2 = o1 + (size_t)np * nout * per_out,
           *dbeta = o2 + (size_t)np * nout * per_out;
    std::vector<double> hb((size_t)np * r);
    std::vector<int> hrow((size_t)np * 2);
    const size_t lds = ss_news_lds(r, s, ncls) * 8;
    auto *kernel = G.mixed ? ss_news_kernel<true> : ss_news_kernel<false>;
    if (lds > 65536)   // the attribute is per device: set on every call (cheap)
      HIPCHK(ctx, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t j0 = 0; j0 < J; j0 += np) {
      const int64_t n = std::min(np, J - j0);
      for (int64_t d = 0; d < n; ++d) {
        const int64_t i = rel_i[j0 + d];
        hrow[d] = (int)rel_t[j0 + d];
        hrow[n + d] = G.mixed && low[i] ? 1 : 0;
        for (int q = 0; q < r; ++q) hb[(size_t)q * n + d] = L[(size_t)q * G.N + i] / sigma2[i];
      }
      HIPCHK(ctx, hipMemcpyAsync(drow.p, hrow.data(), (size_t)n * 2 * 4, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipMemcpyAsync(dbeta, hb.data(), (size_t)n * r * 8, hipMemcpyHostToDevice, st));
      double *wfl = o1, *wal = o1 + (size_t)n * per_out, *wft = o2, *wat = o2 + (size_t)n * per_out;
      {
        Scope sc(ctx, DFM_KC_FACTORS);
        const NewsArgs na{Tt, t_lo, r, s, (int)n, nw, (const int *)drow.p, dbeta, (const double *)drec.p,
                          (const double *)dcst.p, cf, wfl, wal};
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, na);
      }
      HIPCHK(ctx, hipGetLastError());
      {
        Scope sc(ctx, DFM_KC_GEMM);
        if (wf) HIPCHK(ctx, launch_ss_transpose(wfl, (int64_t)per_out, n, wft, st));
        if (agg) HIPCHK(ctx, launch_ss_transpose(wal, (int64_t)per_out, n, wat, st));
      }
      if (wf) HIPCHK(ctx, hipMemcpyAsync(wf + (size_t)j0 * per_out, wft, (size_t)n * per_out * 8, hipMemcpyDeviceToHost, st));
      if (agg) HIPCHK(ctx, hipMemcpyAsync(wa + (size_t)j0 * per_out, wat, (size_t)n * per_out * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));   // hrow and hb are reused
    }
    return 0;
  }
};

const char *news_why(SsNewsBad why) {
  switch (why) {
    case SS_NEWS_RANGE: return "lies outside the panel";
    case SS_NEWS_UNSORTED: return "comes before its predecessor: the list must be sorted by (t, i)";
    case SS_NEWS_DUPLICATE: return "is listed twice";
    case SS_NEWS_DROPPED: return "is observed in X_old and NaN in X_new: the old observed set must lie in the new one";
    case SS_NEWS_NOT_NEW: return "is listed but is no release (observed in X_new and NaN in X_old)";
    case SS_NEWS_MISSING: return "is a release (observed in X_new, NaN in X_old) that the list leaves out";
    default: return "";
  }
}

}  // namespace

extern "C" int dfm_ss_news(dfm_ctx *ctx, const double *X_old, const double *X_new, int64_t T, int64_t N, int64_t ldx,
                           const dfm_ss_params *params, const dfm_ss_mf *mf, const dfm_ss_news_spec *spec, int64_t J,
                           const int64_t *rel_t, const int64_t *rel_i, const dfm_ss_news_out *out) {
  const char *who = "dfm_ss_news";
  if (!ctx) return -1;
  if (!params || !spec || !out) return fail(ctx, -2, "%s: bad arguments", who);
  if (!X_old || !X_new || T < 1 || N < 1 || ldx < T) return fail(ctx, -2, "%s: bad panel layout", who);
  if (ss_news_check_args(J, rel_t && rel_i, T, spec->horizon, spec->t_lo, spec->pass_releases))
    return fail(ctx, -2, "%s: bad arguments (0 <= J <= 2^24 with both lists, 0 <= horizon, 0 <= t_lo < T + horizon, "
                "pass_releases >= 0)", who);
  int L = 0;
  if (mf)
    if (int rc = ss_mf_args(ctx, who, mf, N, true, params->r, params->p, "r, p, n_w", &L)) return rc;
  int64_t where = -1;
  if (int rc = ss_check_params(N, params->r, params->p, params->lambda, params->sigma2, params->A, params->Q,
                               params->a0, params->P0, &where))
    return ss_param_error(ctx, who, rc, where);
  int64_t bt = -1, bi = -1;
  if (const SsNewsBad why = ss_news_check_releases(X_old, X_new, T, N, ldx, J, rel_t, rel_i, &bt, &bi))
    return fail(ctx, -2, "%s: the entry (t = %lld, i = %lld) (0-based) %s", who, (long long)bt, (long long)bi,
                news_why(why));
  // ---- the model's state: the padded one with a low series, the plain one without
  std::vector<dfm_ss_params> padded;
  std::vector<double> Apad;
  const dfm_ss_params *q = params;
  if (L) {
    if (ss_mf_pad_params(params, 1, params->r, params->p, L, padded, Apad) >= 0) return fail(ctx, -2, "%s: bad arguments", who);
    q = &padded[0];
  }
  const dfm_ss_mf *mfu = L ? mf : nullptr;
  const SsParams pr{q->r, q->p, q->lambda, q->sigma2, q->A, q->Q, q->a0, q->P0};
  const int r = pr.r, h = spec->horizon;
  const int64_t Tt = T + h;
  // ---- the three smooths; the revised one's rows are read below whether the caller wants them or not
  std::vector<double> Xrev((size_t)T * N), srev, arev;
  ss_news_revised(X_old, X_new, T, N, ldx, Xrev.data());
  double *sm_rev = out->smoothed_rev, *ag_rev = mfu ? out->smoothed_agg_rev : nullptr;
  if (J > 0 && !sm_rev) srev.resize((size_t)Tt * r), sm_rev = srev.data();
  if (J > 0 && mfu && !ag_rev) arev.resize((size_t)Tt * r), ag_rev = arev.data();
  NewsRun run;
  run.ctx = ctx, run.J = J, run.pass_releases = spec->pass_releases, run.t_lo = spec->t_lo;
  run.rel_t = rel_t, run.rel_i = rel_i, run.L = pr.L, run.sigma2 = pr.sigma2;
  if (mfu) run.low = mfu->low, run.w = mfu->w, run.nw = mfu->n_w;
  run.wf = out->weights_f, run.wa = out->weights_agg;
  const bool weights = J > 0 && (run.wf || (mfu && run.wa));
  DeviceShare gate(ctx->device);
  auto smooth = [&](const double *X, int64_t ld, double *sm, double *ag, SsAfter *after) {
    return ss_smooth_core(ctx, X, 1, T, N, ld, ld * N, false, pr, h, nullptr, sm, nullptr, nullptr, nullptr, mfu,
                          mfu ? ag : nullptr, after, who);
  };
  if (out->smoothed_old || (mfu && out->smoothed_agg_old))
    if (int rc = smooth(X_old, ldx, out->smoothed_old, out->smoothed_agg_old, nullptr)) return rc;
  if (sm_rev || ag_rev)
    if (int rc = smooth(Xrev.data(), T, sm_rev, ag_rev, nullptr)) return rc;
  if (weights || out->smoothed_new || (mfu && out->smoothed_agg_new))
    if (int rc = smooth(X_new, ldx, out->smoothed_new, out->smoothed_agg_new, weights ? &run : nullptr)) return rc;
  // ---- the news: I_j = x_new - lambda' Z_c a_t|rev
  for (int64_t j = 0; j < J; ++j) {
    const int64_t t = rel_t[j], i = rel_i[j];
    const double *a = (mfu && mfu->low[i] ? ag_rev : sm_rev) + (size_t)t * r;
    double f = 0.0;
    for (int k = 0; k < r; ++k) f = fma(pr.L[(size_t)k * N + i], a[k], f);
    if (out->release_forecast) out->release_forecast[j] = f;
    if (out->news) out->news[j] = X_new[i * ldx + t] - f;
  }
  return 0;
}
