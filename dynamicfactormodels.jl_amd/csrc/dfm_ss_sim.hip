// dfm_ss_sim.hip — the simulation smoother of Durbin & Koopman (2002) on top of
// the state-space pass: D joint draws of the factor path given the observed
// entries of one panel (dfm_ss_simulate; the algorithm, the layout of the
// normals and the return codes are stated in include/dfm.h).
//
// The smoother's own launches run once on the panel (ss_smooth_core of
// dfm_ss.hip, which hands over what they leave on the device and the geometry
// they ran at), then
//   ss_gain_kernel          one workgroup per row t, the rows independent: the
//                           row's K chunks added in the filter's order, K_t by
//                           the filter's Gauss-Jordan inverse of G, J_t by the
//                           smoother's Cholesky inverse of P_{t+1|t}, and R_t,
//                           into one record per row
//   ss_sim_kernel           one lane per draw, one wave per workgroup: alpha+,
//                           b* and c forwards, c_t|T backwards; a draw's state
//                           lives in LDS columns [k][lane], the row's record is
//                           staged in LDS once per wave and read by broadcast
//   ss_sim_transpose_kernel the pass's draws from the lanes' layout
//                           [t][k][draw] to the caller's [draw][t][k]
// The covariance recursion is never repeated: a draw is a mean-only recursion
// of about 3 r s multiply-adds per row.  No lane reads another lane's values,
// so a draw depends on neither D, its position nor its pass, and a NaN among
// its normals stays in it.
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_ss_lane.h"

namespace {

// A row's record: n_t > 0 (1.0 / 0.0), b_t (r), C_t (r x r), R_t (r x r, lower),
// K_t (s x r) — what the forward pass reads — then J_t (s x s), all row-major.
__host__ __device__ inline int ss_rec_fwd(int r, int s) { return 1 + r + 2 * r * r + s * r; }
__host__ __device__ inline int ss_rec_len(int r, int s) { return ss_rec_fwd(r, s) + s * s; }

struct SsGainArgs {
  int T, Tt, r, s, KS, Tpad, NCP;
  const double *part, *ws;   // as ss_filter_kernel left them (one panel)
  const double *Tm, *P0;     // s x s row-major
  double *rec;               // [Tt][ss_rec_len]
};

// Row blockIdx.x.  Matrices in LDS with row stride SS_LS, the products on the
// companion matrix as in ss_filter_kernel / ss_smoother_kernel.  P_t|t-1 of
// row 0 is P0 (the filter keeps the predictions of rows >= 1 only).  The
// filter and the smoother have inverted the same matrices by the same steps
// and reported a singular one before this runs: the flag here is not read.
__global__ __launch_bounds__(256) void ss_gain_kernel(SsGainArgs g) {
  __shared__ double lds[6 * SS_MAT + 32 + 64 + 160 + 4];
  __shared__ int ibad, ipiv;
  double *Tm = lds, *P = Tm + SS_MAT, *B1 = P + SS_MAT, *Lw = B1 + SS_MAT, *Tw = Lw + SS_MAT, *GA = Tw + SS_MAT;
  double *colj = GA + SS_MAT, *rowj = colj + 32, *crow = rowj + 64, *sc = crow + 160;
  const int tid = threadIdx.x, t = blockIdx.x;
  const int T = g.T, Tt = g.Tt, r = g.r, s = g.s, ss = s * s;
  const int nC = r * (r + 1) / 2, cn = nC + r + 1;
  const double *Pu = g.ws + (int64_t)Tt * 2 * s, *Pp = Pu + (int64_t)Tt * ss;
  const double *Pprev = t == 0 ? g.P0 : Pp + (int64_t)t * ss;
  double *rec = g.rec + (int64_t)t * ss_rec_len(r, s);
  double *rb = rec + 1, *rC = rb + r, *rR = rC + r * r, *rK = rR + r * r, *rJ = rK + s * r;
  const int64_t pstep = (int64_t)g.Tpad * g.NCP;
  for (int c = tid; c < nC + r + 3; c += 256) {
    double v = 0.0;
    if (t < T)
      for (int k = 0; k < g.KS; ++k) v += g.part[k * pstep + (int64_t)t * g.NCP + c];
    crow[c] = v;
  }
  for (int e = tid; e < ss; e += 256) {
    Tm[(e / s) * SS_LS + e % s] = g.Tm[e];
    P[(e / s) * SS_LS + e % s] = Pprev[e];
  }
  if (tid == 0) ibad = 0;
  __syncthreads();
  const bool obs = crow[cn] > 0.0;
  auto C = [&](int i, int j) { return crow[ss_tri(i, j)]; };
  if (tid == 0) rec[0] = obs ? 1.0 : 0.0;
  if (obs) {
    for (int e = tid; e < r * r; e += 256) {   // G = I + C Pff beside the identity
      const int i = e / r, j = e % r;
      double v = i == j ? 1.0 : 0.0;
      for (int k = 0; k < r; ++k) v = fma(C(i, k), P[k * SS_LS + j], v);
      GA[i * SS_LS + j] = v;
      GA[i * SS_LS + r + j] = i == j ? 1.0 : 0.0;
      Lw[i * SS_LS + j] = 0.0;
    }
    __syncthreads();
    if (tid == 0) {   // R_t in Lw: the rule of ss_psd_cholesky
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
    for (int e = tid; e < s * r + r * r + r; e += 256) {
      if (e < s * r) {   // K = Pf G^-1
        const int i = e / r, j = e % r;
        double v = 0.0;
        for (int k = 0; k < r; ++k) v = fma(P[i * SS_LS + k], GA[k * SS_LS + r + j], v);
        rK[e] = v;
      } else if (e < s * r + r * r) {
        const int q = e - s * r, i = q / r, j = q % r;
        rC[q] = C(i, j);
        rR[q] = Lw[i * SS_LS + j];
      } else {
        rb[e - s * r - r * r] = crow[nC + e - s * r - r * r];
      }
    }
  } else {
    for (int e = tid; e < ss_rec_fwd(r, s) - 1; e += 256) rb[e] = 0.0;
  }
  if (t == Tt - 1) {
    for (int e = tid; e < ss; e += 256) rJ[e] = 0.0;
    return;
  }
  __syncthreads();   // P and Lw are read
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

struct SsSimArgs {
  int Tt, r, s, n;       // n: the pass's draws
  int64_t ldz;
  const double *z;       // the pass's first draw: draw d's entry e at z[e ldz + d]
  const double *rec;     // ss_gain_kernel's records
  const double *cst;     // a0 (s), L0 (s x s), the companion matrix's first r rows (r x s), Lq (r x r), row-major
  double *cf, *out;      // c_t|t [Tt][s][n] and the draws [Tt][r][n]
};

constexpr int SS_SIM_PRE = 17;   // 64 SS_SIM_PRE >= the forward record and J_t at r = 16, s = 32

// LDS doubles of ss_sim_kernel: the companion rows, Lq, one staged record, and
// the columns of alpha+ (s), c (s) and the work vector (max(s, 2 r)).
inline size_t ss_sim_lds(int r, int s) {
  return (size_t)(r * s + r * r + std::max(ss_rec_fwd(r, s), s * s) + (2 * s + std::max(s, 2 * r)) * 64);
}

// Draw blockIdx.x * 64 + lane of the pass.  Element k of a lane's vector is at
// [k * 64 + lane] of its LDS region: a wave's access is one conflict-free row,
// and every read of the staged record is a broadcast.  What the next row reads
// from global memory — its record, and the lane's own normals (forwards) or
// c_t|t (backwards) — is fetched into registers while this row is computed, so
// a row waits for no load of its own; the two barriers per row fence the
// staging buffer (the workgroup is one wave).  A lane past the pass's last
// draw reads zeros for its normals and stores nothing.
__global__ __launch_bounds__(64) void ss_sim_kernel(SsSimArgs g) {
  extern __shared__ __attribute__((aligned(16))) double sim_lds[];
  const int Tt = g.Tt, r = g.r, s = g.s, n = g.n, lane = threadIdx.x;
  const int nf = ss_rec_fwd(r, s), nrec = nf + s * s, ss = s * s;
  double *Tmr = sim_lds, *Lq = Tmr + r * s, *st = Lq + r * r;
  double *A = st + (nf > ss ? nf : ss) + lane, *Cc = A + s * 64, *W = Cc + s * 64;   // this lane's columns
  const int64_t d = (int64_t)blockIdx.x * 64 + lane;
  const bool act = d < n;
  const double *zc = g.z + (act ? d : 0);
  auto zat = [&](int64_t e) { return act ? zc[e * g.ldz] : 0.0; };
  const double *a0 = g.cst, *L0 = a0 + s;
  for (int e = lane; e < r * s + r * r; e += 64) Tmr[e] = g.cst[s + ss + e];   // Tmr and Lq are adjacent on both sides
  double pre[SS_SIM_PRE];
  auto fetch = [&](const double *src, int len) {
#pragma unroll
    for (int q = 0; q < SS_SIM_PRE; ++q) {
      const int e = lane + 64 * q;
      pre[q] = e < len ? src[e] : 0.0;
    }
  };
  auto stage = [&](int len) {
    __syncthreads();   // the previous record is read
#pragma unroll
    for (int q = 0; q < SS_SIM_PRE; ++q) {
      const int e = lane + 64 * q;
      if (e < len) st[e] = pre[q];
    }
    __syncthreads();
  };
  double lp[32], lo[16];   // the lane's own next row: 2 r normals or s entries of c_t|t; r entries of the output row
  auto lfetch = [&](const double *base, int64_t step, int cnt) {
#pragma unroll
    for (int q = 0; q < 32; ++q) lp[q] = (act && q < cnt) ? base[q * step] : 0.0;
  };
  auto lput = [&](double *x, int cnt) {
#pragma unroll
    for (int q = 0; q < 32; ++q)
      if (q < cnt) x[q * 64] = lp[q];
  };
  // x <- Tm x on a lane's column: the first r rows by dot products into W, the rest a shift
  auto advance = [&](double *x) {
    for (int i = 0; i < r; ++i) W[i * 64] = sim_dot<false>(0.0, Tmr + i * s, x, s);
    for (int i = s - 1; i >= r; --i) x[i * 64] = x[(i - r) * 64];
    for (int i = 0; i < r; ++i) x[i * 64] = W[i * 64];
  };
  for (int i = 0; i < s; ++i) Cc[i * 64] = 0.0;
  fetch(g.rec, nf);
  lfetch(zc + s * g.ldz, g.ldz, 2 * r);
  // ---------------------------------------------------------------- forwards
  for (int t = 0; t < Tt; ++t) {
    stage(nf);
    if (t == 0) {   // alpha+_0 = a0 + L0 z0
      for (int k = 0; k < s; ++k) W[k * 64] = zat(k);
      for (int i = 0; i < s; ++i) A[i * 64] = sim_dot<false>(a0[i], L0 + i * s, W, i + 1);
    } else {
      advance(A);
    }
    lput(W, 2 * r);   // u_t at W[0, r), zeta_t at W[r, 2 r)
    if (t + 1 < Tt) {
      fetch(g.rec + (int64_t)(t + 1) * nrec, nf);
      lfetch(zc + (s + 2 * (int64_t)r * (t + 1)) * g.ldz, g.ldz, 2 * r);
    } else if (Tt >= 2) {
      fetch(g.rec + (int64_t)(Tt - 2) * nrec + nf, ss);
    }
    if (t > 0)      // alpha+_t = Tm alpha+_{t-1} + [Lq u_t; 0]
      for (int i = 0; i < r; ++i) A[i * 64] = sim_dot<false>(A[i * 64], Lq + i * r, W, i + 1);
    if (act)
      for (int i = 0; i < r; ++i) g.out[((int64_t)t * r + i) * n + d] = A[i * 64];
    if (st[0] != 0.0) {
      const double *b = st + 1, *C = b + r, *R = C + r * r, *K = R + r * r;
      for (int i = 0; i < r; ++i) {
        double v = sim_dot<true>(b[i], C + i * r, A, r);   // b* = b - C f+ - R zeta
        v = sim_dot<true>(v, R + i * r, W + r * 64, i + 1);
        W[i * 64] = sim_dot<true>(v, C + i * r, Cc, r);    // b* - C c[:r]
      }
      for (int i = 0; i < s; ++i) Cc[i * 64] = sim_dot<false>(Cc[i * 64], K + i * r, W, r);
    }
    if (t == Tt - 1) break;
    if (act)
      for (int i = 0; i < s; ++i) g.cf[((int64_t)t * s + i) * n + d] = Cc[i * 64];
    advance(Cc);
  }
  // --------------------------------------------------------------- backwards
  if (act)
    for (int i = 0; i < r; ++i) g.out[((int64_t)(Tt - 1) * r + i) * n + d] += Cc[i * 64];
  const double *cfd = g.cf + (act ? d : 0);
  double *outd = g.out + (act ? d : 0);
  if (Tt >= 2) lfetch(cfd + (int64_t)(Tt - 2) * s * n, n, s);
  for (int t = Tt - 2; t >= 0; --t) {
    stage(ss);   // J_t
    lput(A, s);  // c_t|t
#pragma unroll
    for (int q = 0; q < 16; ++q) lo[q] = (act && q < r) ? outd[((int64_t)t * r + q) * n] : 0.0;   // f+_t
    if (t >= 1) {
      fetch(g.rec + (int64_t)(t - 1) * nrec + nf, ss);
      lfetch(cfd + (int64_t)(t - 1) * s * n, n, s);
    }
    for (int i = 0; i < s; ++i) {   // c_{t+1|T} - Tm c_t|t
      const double v = i < r ? sim_dot<false>(0.0, Tmr + i * s, A, s) : A[(i - r) * 64];
      W[i * 64] = Cc[i * 64] - v;
    }
    for (int i = 0; i < s; ++i) Cc[i * 64] = sim_dot<false>(A[i * 64], st + i * s, W, s);
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (act && q < r) outd[((int64_t)t * r + q) * n] = lo[q] + Cc[q * 64];
  }
}

// in: rows x n (the draw fastest) -> out: n x rows, by 32 x 32 tiles through LDS;
// tile blockIdx.x % nxt along the draws, blockIdx.x / nxt along the rows.
__global__ __launch_bounds__(256) void ss_sim_transpose_kernel(const double *__restrict__ in, int64_t rows, int64_t n,
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

// The draws, from what the smoother's launches left on the device.
struct SimRun : SsAfter {
  dfm_ctx *ctx = nullptr;
  int64_t D = 0, ldz = 0, pass_draws = 0;
  const double *z = nullptr;
  bool z_dev = false;
  double *draws = nullptr;
  std::vector<double> Lq;   // r x r row-major, the Cholesky factor of Q

  int run(const SsKept &k) override {
    const SsGeom &G = k.g;
    const int Tt = G.Tt, r = G.r, s = G.s, ss = s * s, nrec = ss_rec_len(r, s);
    const int64_t nz = ss_sim_nz(Tt, r, s);
    hipStream_t st = ctx->stream;
    // ---- the constants: a0, L0, the companion matrix's first r rows, Lq
    std::vector<double> hc((size_t)s + ss + r * s + r * r);
    std::copy(k.ha0, k.ha0 + s, hc.begin());
    ss_psd_cholesky(k.hP0, s, &hc[s]);
    std::copy(k.hTm, k.hTm + r * s, &hc[(size_t)s + ss]);
    std::copy(Lq.begin(), Lq.end(), &hc[(size_t)s + ss + r * s]);
    StreamBuf dcst, drec, dwork, dz;
    HIPCHK(ctx, dcst.alloc(hc.size() * 8, st));
    HIPCHK(ctx, hipMemcpyAsync(dcst.p, hc.data(), hc.size() * 8, hipMemcpyHostToDevice, st));
    // ---- the gains, once
    HIPCHK(ctx, drec.alloc((size_t)Tt * nrec * 8, st));
    {
      Scope sc(ctx, DFM_KC_OLS);
      const SsGainArgs ga{G.T, Tt, r, s, G.KS, G.Tpad, G.NCP, k.part, k.ws, k.dTm, k.dP0, (double *)drec.p};
      hipLaunchKernelGGL(ss_gain_kernel, dim3((unsigned)Tt), dim3(256), 0, st, ga);
    }
    HIPCHK(ctx, hipGetLastError());
    // ---- the draws, in passes
    const int64_t np = ss_sim_draws_per_pass(Tt, r, s, D, pass_draws, !z_dev);
    const size_t per_cf = (size_t)Tt * s, per_out = (size_t)Tt * r;
    HIPCHK(ctx, dwork.alloc((size_t)np * (per_cf + 2 * per_out) * 8, st));
    if (!z_dev) HIPCHK(ctx, dz.alloc((size_t)np * nz * 8, st));
    double *cf = (double *)dwork.p, *o1 = cf + (size_t)np * per_cf, *o2 = o1 + (size_t)np * per_out;
    const size_t lds = ss_sim_lds(r, s) * 8;
    for (int64_t d0 = 0; d0 < D; d0 += np) {
      const int64_t n = std::min(np, D - d0);
      const double *zp = z + d0;
      int64_t ld = ldz;
      if (!z_dev) {
        HIPCHK(ctx, hipMemcpy2DAsync(dz.p, (size_t)n * 8, zp, (size_t)ldz * 8, (size_t)n * 8, (size_t)nz,
                                     hipMemcpyHostToDevice, st));
        zp = (const double *)dz.p;
        ld = n;
      }
      {
        Scope sc(ctx, DFM_KC_FACTORS);
        const SsSimArgs sa{Tt, r, s, (int)n, ld, zp, (const double *)drec.p, (const double *)dcst.p, cf, o1};
        hipLaunchKernelGGL(ss_sim_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, sa);
      }
      HIPCHK(ctx, hipGetLastError());
      {
        Scope sc(ctx, DFM_KC_GEMM);
        HIPCHK(ctx, launch_ss_transpose(o1, (int64_t)per_out, n, o2, st));
      }
      HIPCHK(ctx, hipMemcpyAsync(draws + (size_t)d0 * per_out, o2, (size_t)n * per_out * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
    }
    return 0;
  }
};

}  // namespace

hipError_t dfm::launch_ss_transpose(const double *in, int64_t rows, int64_t n, double *out, hipStream_t st) {
  const int nxt = (int)((n + 31) / 32);
  const int64_t nyt = (rows + 31) / 32;
  hipLaunchKernelGGL(ss_sim_transpose_kernel, dim3((unsigned)(nxt * nyt)), dim3(256), 0, st, in, rows, n, nxt, out);
  return hipGetLastError();
}

extern "C" int dfm_ss_simulate(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx,
                               const dfm_ss_params *params, const dfm_ss_sim_spec *spec, int64_t D, const double *z,
                               int64_t ldz, double *draws, double *smoothed, double *smoothed_cov, double *loglik) {
  const char *who = "dfm_ss_simulate";
  if (!ctx) return -1;
  if (!params || !spec) return fail(ctx, -2, "%s: bad arguments", who);
  if (ss_sim_check_args(D, z != nullptr, draws != nullptr, ldz, spec->horizon, spec->pass_draws))
    return fail(ctx, -2, "%s: bad arguments (1 <= D <= 2^24, z and draws given, ldz >= D, pass_draws >= 0)", who);
  int64_t where = -1;
  const int r = params->r;
  int rc = ss_check_params(N, r, params->p, params->lambda, params->sigma2, params->A, params->Q, params->a0,
                           params->P0, &where);
  if (rc) return ss_param_error(ctx, who, rc, where);
  SimRun run;
  run.Lq.resize((size_t)r * r);   // the filter reads Q's lower triangle, row-major
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) run.Lq[i * r + j] = j <= i ? params->Q[(size_t)j * r + i] : 0.0;
  if (!ss_cholesky(run.Lq.data(), r)) return ss_param_error(ctx, who, SS_E_SINGULAR, -1);
  run.ctx = ctx;
  run.D = D;
  run.z = z;
  run.ldz = ldz;
  run.z_dev = spec->z_dev != 0;
  run.pass_draws = spec->pass_draws;
  run.draws = draws;
  DeviceShare gate(ctx->device);
  const SsParams pr{r, params->p, params->lambda, params->sigma2, params->A, params->Q, params->a0, params->P0};
  return ss_smooth_core(ctx, X, 1, T, N, ldx, ldx * N, spec->dev != 0, pr, spec->horizon, nullptr, smoothed,
                        smoothed_cov, loglik, nullptr, nullptr, nullptr, &run, who);
}
