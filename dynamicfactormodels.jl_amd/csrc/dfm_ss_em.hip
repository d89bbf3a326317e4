// dfm_ss_em.hip — the quasi-ML EM of the state-space factor model (dfm_ss_em,
// dfm_ss_em_mf, dfm_ss_em_blocks; stated in include/dfm.h).  Every panel of the batch has its own
// parameter block and an `active` flag; an iteration is the E-step (ss_estep of
// dfm_ss.hip, which also leaves S11, S10, S00 and the M-step's operand rows), then
//   ss_mstep_kernel      the transpose of the collapse: [mask | zero-filled
//                        panel]' against those rows on the same tile, K = T in
//                        chunks of SS_KC rows: S_i, g_i, n_i, q_i per series
//   ss_loadings_kernel   per series lambda_i, sigma^2_i and the next pass's
//                        collapse operands
//   ss_transition_kernel per panel A, Q, the companion matrix, a0 / P0
// and ss_empty_column_kernel looks once, before the first pass, for a column
// of a device-resident panel without an observed entry.
// Mixed frequency: the <true> instantiations read and write a series' own
// class's columns and regress the VAR on its own lags.
// Factor blocks (dfm_ss_em_blocks): the <., true> instantiations of the last two
// keep Lambda's restricted entries at zero and A, Q block-diagonal.
// No kernel uses an atomic, and the K split depends on T alone: panel b of a
// batch is bit-identical to a call on panel b alone.
#include "dfm_host.h"
#include "dfm_small.h"
#include "dfm_ss_host.h"
#include "dfm_tile.h"

namespace {

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

// Series blockIdx.x * SS_LB + threadIdx.x of panel blockIdx.y: the K chunks of
// its row added in their order, lambda_i = S_i^-1 g_i by a Cholesky in the
// thread's own LDS column, sigma^2_i = (q_i - lambda_i'g_i) / n_i, and the next
// pass's operands of the collapse.  status ([panel][N]): 0, or 1 S_i not
// positive definite, 2 sigma^2_i not positive, 3 no observed entry — the
// parameters of such a series are left as they were.
// MF: low[i] names the series' class; it reads that class's group of its row
// and writes the collapse operands at that class's columns.
// R (factor blocks): bit j of free[i] says that the series loads on factor j.
// Row and column j of S_i become e_j and g_ij zero for the others, so every
// lane keeps the trip counts of the r x r system: the solve leaves the free
// sub-system's solution and lambda_ij = 0 there, which is written as 0.0
// into Lambda and the collapse operands.
template <bool MF, bool R>
__global__ __launch_bounds__(SS_LB) void ss_loadings_kernel(const double *__restrict__ pm, int N, int Nr, int r, int NCP,
                                                            int KS, const int *__restrict__ active, SsBlock L,
                                                            double *__restrict__ par, int *__restrict__ status,
                                                            const uint8_t *__restrict__ low,
                                                            const uint16_t *__restrict__ free) {
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
  unsigned fm = 0xffffu;
  if constexpr (R) {
    fm = free[i];
    for (int a = 0; a < r; ++a) {
      const bool fa = (fm >> a) & 1;
      if (!fa) W(nC + a) = 0.0;
      for (int c = 0; c <= a; ++c)
        if (!fa || !((fm >> c) & 1)) W(ss_tri(a, c)) = a == c ? 1.0 : 0.0;
    }
  }
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
    const bool fa = !R || ((fm >> a) & 1);
    const double la = fa ? W(y + a) : 0.0;
    for (int c = 0; c <= a; ++c) wm[co + ss_tri(a, c)] = (fa && (!R || ((fm >> c) & 1))) ? la * W(y + c) / v : 0.0;
    wv[co + nC + a] = fa ? la / v : 0.0;
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
// R (factor blocks, bo): one block after the other, rows G = its factors and
// columns c = its factors at every lag of the VAR: S00[c, c] and S10[G, c]
// gathered into the LDS matrices, A[G, c] = S10[G, c] S00[c, c]^-1 and Q[G, G]
// as above; the rest of A's rows and of Q is written as zero.
template <bool MF, bool R>
__global__ __launch_bounds__(256) void ss_transition_kernel(const double *__restrict__ mom, int T, int N, int r, int s, int rp,
                                                            int update_init, const int *__restrict__ active, SsBlock L,
                                                            double *__restrict__ par, const int *__restrict__ status,
                                                            int *__restrict__ mflag, int *__restrict__ mcol, SsBlockOff bo) {
  __shared__ double lds[6 * SS_MAT + (R ? 2 * SS_RMAX * SS_LS : 0)];
  __shared__ int first[256];
  __shared__ int ibad;
  double *S00 = lds, *Si = S00 + SS_MAT, *Lw = Si + SS_MAT, *Tw = Lw + SS_MAT, *S10 = Tw + SS_MAT, *Am = S10 + SS_MAT;
  const int tid = threadIdx.x, b = blockIdx.x, ss = s * s;
  if (!active[b]) return;
  const double *m = mom + (int64_t)b * SS_MOM;
  double *P = par + (int64_t)b * L.stride;
  const int n = MF ? rp : s;
  if constexpr (!R) {
    for (int e = tid; e < n * n; e += 256) S00[(e / n) * SS_LS + e % n] = m[SS_M00 + (e / n) * s + e % n];
    for (int e = tid; e < r * n; e += 256) S10[(e / n) * SS_LS + e % n] = m[SS_M10 + (e / n) * s + e % n];
  }
  int f = N;
  for (int i = tid; i < N; i += 256)
    if (status[(int64_t)b * N + i] && i < f) f = i;
  first[tid] = f;
  if (tid == 0) ibad = 0;
  if constexpr (R) {
    double *AF = lds + 6 * SS_MAT, *QF = AF + SS_RMAX * SS_LS;   // A's rows and Q of all blocks, zero outside them
    for (int e = tid; e < 2 * SS_RMAX * SS_LS; e += 256) AF[e] = 0.0;
    const int pv = n / r;   // the VAR's own lags
    for (int g = 0; g < bo.nb; ++g) {
      const int o = bo.off[g], rg = bo.off[g + 1] - o, ng = rg * pv;
      auto col = [&](int c) { return (c / rg) * r + o + c % rg; };   // the block's column c among the state's
      __syncthreads();   // the previous block's matrices are read
      for (int e = tid; e < ng * ng; e += 256) S00[(e / ng) * SS_LS + e % ng] = m[SS_M00 + col(e / ng) * s + col(e % ng)];
      for (int e = tid; e < rg * ng; e += 256) S10[(e / ng) * SS_LS + e % ng] = m[SS_M10 + (o + e / ng) * s + col(e % ng)];
      __syncthreads();
      dfm::block_spd_inverse(S00, Si, Lw, Tw, ng, SS_LS, &ibad);
      for (int e = tid; e < rg * ng; e += 256) {
        const int i = e / ng, j = e % ng;
        double v = 0.0;
        for (int k = 0; k < ng; ++k) v = fma(S10[i * SS_LS + k], Si[k * SS_LS + j], v);
        Am[i * SS_LS + j] = v;
        AF[(o + i) * SS_LS + col(j)] = v;
      }
      __syncthreads();
      for (int e = tid; e < rg * rg; e += 256) {
        const int i = e / rg, j = e % rg;
        double v = m[SS_M11 + (o + i) * r + o + j];
        for (int k = 0; k < ng; ++k) v = fma(-Am[i * SS_LS + k], S10[j * SS_LS + k], v);
        Lw[i * SS_LS + j] = v / (double)(T - 1);
      }
      __syncthreads();
      for (int e = tid; e < rg * rg; e += 256) {
        const int i = e / rg, j = e % rg;
        QF[(o + i) * SS_LS + o + j] = 0.5 * (Lw[i * SS_LS + j] + Lw[j * SS_LS + i]);
      }
    }
    __syncthreads();
    if (!ibad) {
      for (int e = tid; e < r * r; e += 256) P[L.oQ + e] = QF[(e / r) * SS_LS + e % r];
      for (int e = tid; e < r * n; e += 256) P[L.oTm + (e / n) * s + e % n] = AF[(e / n) * SS_LS + e % n];
    }
  } else {
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
    }
  }
  if (!ibad) {
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

int dfm::ss_blocks_args(dfm_ctx *ctx, const char *who, const dfm_ss_blocks *blocks, int64_t N, int r, bool *trivial,
                        SsBlocks *bl, std::vector<uint16_t> &free) {
  *trivial = false;
  if (!blocks) return fail(ctx, -2, "%s: the factor blocks are missing", who);
  int64_t where = -1;
  switch (ss_blocks_check(blocks->n_blocks, blocks->block_r, blocks->member, N, r, &where)) {
    case SS_BLK_OK: break;
    case SS_BLK_NULL: return fail(ctx, -2, "%s: the blocks' sizes or their membership matrix are missing", who);
    case SS_BLK_COUNT: return fail(ctx, -2, "%s: n_blocks = %d is outside 1..16", who, (int)blocks->n_blocks);
    case SS_BLK_SIZE: return fail(ctx, -2, "%s: block %lld (0-based) has a size < 1", who, (long long)where);
    case SS_BLK_SUM:
      return fail(ctx, -2, "%s: the blocks' sizes sum to %lld, the model has r = %d factors", who, (long long)where, r);
    case SS_BLK_SERIES:
      return fail(ctx, -2, "%s: column %lld (0-based) is a member of no block", who, (long long)where);
    case SS_BLK_EMPTY: return fail(ctx, -2, "%s: block %lld (0-based) has no member", who, (long long)where);
  }
  if (ss_blocks_trivial(blocks->n_blocks, blocks->member, N)) {
    *trivial = true;
    return 0;
  }
  if (r > SS_RMAX) return ss_param_error(ctx, who, SS_E_LIMIT, -1);
  int off[SS_BMAX + 1];
  ss_blocks_offsets(blocks->n_blocks, blocks->block_r, off);
  bl->o.nb = blocks->n_blocks;
  for (int g = 0; g <= blocks->n_blocks; ++g) bl->o.off[g] = (uint8_t)off[g];
  free.resize((size_t)N);
  ss_blocks_free_mask(blocks->n_blocks, off, blocks->member, N, free.data());
  bl->free = free.data();
  return 0;
}

// The EM over M panels (include/dfm.h).  The panel and the starts go up once;
// per iteration one read-back (logliks and flags) decides which panels stop,
// and the `active` flags go back; the rest crosses the bus at the end.
int dfm::ss_em_core(dfm_ctx *ctx, const char *who, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx,
                    int64_t stride, bool dev, const dfm_ss_params *starts, int64_t n_start, int max_iter, double tol, bool update_init,
                    int h, const dfm_ss_em_out &out, dfm_ss_em_info *info, const dfm_ss_mf *mf, int p_var,
                    const SsBlocks *blocks) {
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
  auto empty = [&](long long pb, long long c) {
    return fail(ctx, -2, "%s: panel %lld: column %lld (0-based) has no observed entry", who, pb, c);
  };
  int64_t ep = -1, ec = -1;
  if (!dev && ss_em_empty_column(X, M, T64, N64, ldx, stride, &ep, &ec)) return empty(ep, ec);
  if (T64 + h > (1 << 24) || M > (1 << 30)) return fail(ctx, -2, "panel too large");
  const SsGeom G = ss_geom((int)T64, h, (int)N64, r, r * p, mf != nullptr);
  const int T = G.T, N = G.N, s = G.s, ss = s * s, Tt = G.Tt, rp = mf ? r * p_var : s;
  const SsBlock B = ss_block(G);
  const size_t blk = (size_t)B.stride, tail = blk - (size_t)B.oTm;
  // ---- the starts' blocks
  std::vector<double> hp((size_t)n_start * blk);
  for (int64_t k = 0; k < n_start; ++k) {
    const dfm_ss_params &q = starts[k];
    const SsParams pr{q.r, q.p, q.lambda, q.sigma2, q.A, q.Q, q.a0, q.P0};
    if (int rc = ss_fill_block(pr, G, B, &hp[(size_t)k * blk], mf ? mf->low : nullptr))
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
  StreamBuf dfree;   // factor blocks: the series' free masks
  SsBlockOff bo{};
  if (blocks) {
    bo = blocks->o;
    HIPCHK(ctx, dfree.alloc((size_t)N * 2, st));
    HIPCHK(ctx, hipMemcpyAsync(dfree.p, blocks->free, (size_t)N * 2, hipMemcpyHostToDevice, st));
  }
  const uint16_t *dfree_mask = (const uint16_t *)dfree.p;
  // ---- panels per pass: everything a panel keeps on the device — the work doubles, its block and its flags
  const size_t per_part = (size_t)G.KS * G.Tpad * G.NCP, per_ws = (size_t)Tt * (2 * (size_t)s + 2 * (size_t)ss),
               per_pm = (size_t)G.KT * G.Nr * G.NCP, per_op = (size_t)T * G.NCP, per_filt = (size_t)T * r,
               per_sm = (size_t)Tt * r, per_cov = (size_t)Tt * r * r, per_agg = mf ? per_sm : 0;
  const size_t per_work = per_part + per_ws + per_pm + per_op + per_filt + per_sm + per_cov + per_agg + SS_MOM + 2,
               per_int = (size_t)N + 4;
  const int64_t mb = ss_panels_per_pass(M, (per_work + blk) * 8 + per_int * 4);
  StreamBuf dpar, dwork, dint;
  SsStage stage{X, ldx, stride, T, N, dev, st};
  HIPCHK(ctx, dpar.alloc((size_t)mb * blk * 8, st));
  HIPCHK(ctx, dwork.alloc((size_t)mb * per_work * 8, st));
  HIPCHK(ctx, dint.alloc((size_t)mb * per_int * 4, st));
  HIPCHK(ctx, stage.alloc(mb));
  double *dp = (double *)dpar.p, *part = (double *)dwork.p, *ws = part + (size_t)mb * per_part,
         *pm = ws + (size_t)mb * per_ws, *opnd = pm + (size_t)mb * per_pm, *dfilt = opnd + (size_t)mb * per_op,
         *dsm = dfilt + (size_t)mb * per_filt, *dcov = dsm + (size_t)mb * per_sm, *mom = dcov + (size_t)mb * per_cov,
         *dll = mom + (size_t)mb * SS_MOM, *dn = dll + mb,   // dll, dn adjacent: one read-back
         *dagg = dn + mb;
  int *eflag = (int *)dint.p, *mflag = eflag + mb, *mcol = mflag + mb, *dact = mcol + mb, *status = dact + mb;
  SsEstep es{};   // a block per panel, the moments wanted
  es.ldx = ldx, es.stride = stride, es.par = dp, es.pstride = B.stride, es.active = dact, es.part = part, es.ws = ws;
  es.filt = dfilt, es.smooth = dsm, es.cov = dcov, es.ll = dll, es.nobs = dn, es.flag = eflag;
  es.opnd = opnd, es.mom = mom;
  es.nw = mf ? mf->n_w : 0, es.w = dw, es.agg = mf ? dagg : nullptr;
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
      if (hempty[i] >= 0) return empty(i, hempty[i]);
  }
  for (int64_t c0 = 0; c0 < M; c0 += mb) {
    const int64_t n = std::min(mb, M - c0);
    HIPCHK(ctx, stage.pass(c0, n, &es.X));
    for (int64_t i = 0; i < n; ++i)
      HIPCHK(ctx, hipMemcpyAsync(dp + (size_t)i * blk, &hp[(size_t)(n_start == 1 ? 0 : c0 + i) * blk], blk * 8,
                                 hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(opnd, 0, (size_t)n * per_op * 8, st));
    HIPCHK(ctx, hipMemsetAsync(dint.p, 0, (size_t)mb * per_int * 4, st));
    std::fill(act.begin(), act.end(), 1);
    HIPCHK(ctx, hipMemcpyAsync(dact, act.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (out.loglik_path)
      std::fill(out.loglik_path + (size_t)c0 * path_ld, out.loglik_path + (size_t)(c0 + n) * path_ld, (double)NAN);
    int64_t nact = n;
    for (int j = 0;; ++j) {
      if (int rc = ss_estep(ctx, G, B, es, n)) return rc;
      HIPCHK(ctx, hipMemcpyAsync(hll.data(), dll, (size_t)mb * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(hflag.data(), eflag, (size_t)3 * mb * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      for (int64_t i = 0; i < n; ++i) {
        if (!act[i]) continue;
        const long long pb = (long long)(c0 + i);
        const int mfl = hflag[(size_t)mb + i], mcl = hflag[(size_t)2 * mb + i], efl = hflag[i];   // M-step flag and column, E-step flag
        if (mfl & 4) return empty(pb, mcl);
        if (mfl & 2)
          return fail(ctx, SS_E_SIGMA, "%s: panel %lld, the M-step giving iteration %d: the idiosyncratic variance of "
                      "column %d (0-based) is not positive", who, pb, j, mcl);
        if (mfl)
          return fail(ctx, SS_E_SINGULAR, "%s: panel %lld, the M-step giving iteration %d: %s not invertible", who, pb, j,
                      (mfl & 8) ? (blocks ? "a block of S00 is" : "S00 is") : "an S_i is");
        if (efl) return ss_estep_error(ctx, who, pb, efl, j);
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
        hipLaunchKernelGGL(mf ? ss_mstep_kernel<true> : ss_mstep_kernel<false>, dim3(G.nrn, G.nct * G.KT, (unsigned)n),
                           dim3(256), 0, st, es.X, ldx, stride, T, N, (const double *)opnd, (const int *)dact, r, G.NCP, G.nct,
                           G.KT, pm);
      }
      HIPCHK(ctx, hipGetLastError());
      {
        Scope sc(ctx, DFM_KC_OLS);
        auto *loadings = blocks ? (mf ? ss_loadings_kernel<true, true> : ss_loadings_kernel<false, true>)
                                : (mf ? ss_loadings_kernel<true, false> : ss_loadings_kernel<false, false>);
        auto *transition = blocks ? (mf ? ss_transition_kernel<true, true> : ss_transition_kernel<false, true>)
                                  : (mf ? ss_transition_kernel<true, false> : ss_transition_kernel<false, false>);
        hipLaunchKernelGGL(loadings, dim3((N + SS_LB - 1) / SS_LB, (unsigned)n), dim3(SS_LB), 0, st, (const double *)pm, N,
                           G.Nr, r, G.NCP, G.KT, (const int *)dact, B, dp, status, dlow, dfree_mask);
        hipLaunchKernelGGL(transition, dim3((unsigned)n), dim3(256), 0, st, (const double *)mom, T, N, r, s, rp,
                           update_init ? 1 : 0, (const int *)dact, B, dp, (const int *)status, mflag, mcol, bo);
      }
      HIPCHK(ctx, hipGetLastError());
    }
    // ---- the pass's results
    const struct { double *host, *dev; size_t per; } outs[] = {
        {out.filtered, dfilt, per_filt}, {out.smoothed, dsm, per_sm}, {out.smoothed_cov, dcov, per_cov},
        {mf ? out.smoothed_agg : nullptr, dagg, per_sm}};
    for (const auto &o : outs)
      if (o.host) HIPCHK(ctx, hipMemcpyAsync(o.host + c0 * o.per, o.dev, (size_t)n * o.per * 8, hipMemcpyDeviceToHost, st));
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

extern "C" {

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
  const char *who = "dfm_ss_em_mf";
  if (!ctx) return -1;
  int max_iter = 0, L = 0;
  double tol = 0.0;
  const bool ok = spec && out && starts && n_start >= 1 &&
                  !ss_em_defaults(spec->max_iter, spec->tol, spec->horizon, &max_iter, &tol);
  const int r = ok ? starts[0].r : 0, p = ok ? starts[0].p : 0;
  if (int rc = ss_mf_args(ctx, who, mf, N, ok, r, p, "r, p, n_w", &L)) return rc;
  if (!L) return dfm_ss_em(ctx, X, M, T, N, ldx, stride, starts, n_start, spec, out, info);
  std::vector<dfm_ss_params> padded;
  std::vector<double> Apad;
  const int64_t k = ss_mf_pad_params(starts, n_start, r, p, L, padded, Apad);
  if (k >= 0) return fail(ctx, -2, "%s: start %lld has another (r, p)", who, (long long)k);
  DeviceShare gate(ctx->device);
  return ss_em_core(ctx, who, X, M, T, N, ldx, stride, spec->dev != 0, padded.data(), n_start, max_iter, tol,
                    spec->update_init != 0, spec->horizon, *out, info, mf, p);
}

int dfm_ss_em_blocks(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *starts, int64_t n_start, const dfm_ss_mf *mf, const dfm_ss_blocks *blocks,
                     const dfm_ss_em_spec *spec, const dfm_ss_em_out *out, dfm_ss_em_info *info) {
  const char *who = "dfm_ss_em_blocks";
  if (!ctx) return -1;
  int max_iter = 0, L = 0;
  double tol = 0.0;
  if (!spec || !out || !starts || n_start < 1 || N < 1 ||
      ss_em_defaults(spec->max_iter, spec->tol, spec->horizon, &max_iter, &tol))
    return fail(ctx, -2, "%s: bad arguments", who);
  const int r = starts[0].r, p = starts[0].p;
  bool trivial = false;
  SsBlocks bl{};
  std::vector<uint16_t> free;
  if (int rc = ss_blocks_args(ctx, who, blocks, N, r, &trivial, &bl, free)) return rc;
  if (trivial)
    return mf ? dfm_ss_em_mf(ctx, X, M, T, N, ldx, stride, starts, n_start, mf, spec, out, info)
              : dfm_ss_em(ctx, X, M, T, N, ldx, stride, starts, n_start, spec, out, info);
  if (mf)
    if (int rc = ss_mf_args(ctx, who, mf, N, true, r, p, "r, p, n_w", &L)) return rc;
  if (int rc = ss_check_dims(r, L ? L : p)) return ss_param_error(ctx, who, rc, -1);
  int off[SS_BMAX + 1];
  for (int g = 0; g <= bl.o.nb; ++g) off[g] = bl.o.off[g];
  for (int64_t k = 0; k < n_start; ++k) {
    const dfm_ss_params &q = starts[k];
    if (q.r != r || q.p != p) return fail(ctx, -2, "%s: start %lld has another (r, p)", who, (long long)k);
    if (!q.lambda || !q.A || !q.Q) return fail(ctx, -2, "%s: bad arguments", who);
    int64_t i = -1, j = -1;
    if (const int which = ss_blocks_check_start(N, r, p, q.lambda, q.A, q.Q, bl.o.nb, off, bl.free, &i, &j))
      return fail(ctx, -2, "%s: start %lld: %s[%lld, %lld] (0-based) is not zero where the blocks restrict it", who,
                  (long long)k, which == 1 ? "lambda" : which == 2 ? "A" : "Q", (long long)i, (long long)j);
  }
  std::vector<dfm_ss_params> padded;
  std::vector<double> Apad;
  if (L && ss_mf_pad_params(starts, n_start, r, p, L, padded, Apad) >= 0) return fail(ctx, -2, "%s: bad arguments", who);
  DeviceShare gate(ctx->device);
  return ss_em_core(ctx, who, X, M, T, N, ldx, stride, spec->dev != 0, L ? padded.data() : starts, n_start, max_iter, tol,
                    spec->update_init != 0, spec->horizon, *out, info, L ? mf : nullptr, L ? p : 0, &bl);
}

}  // extern "C"
