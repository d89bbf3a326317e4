// dfm_internal.h — the one declaration of every libdfm symbol that one .hip
// file defines and another uses, grouped by the defining file.  Every .hip
// includes it; default arguments live here only.  (What only dfm_eig.hip and
// dfm_fact.hip share is in their private dfm_eig.h.)
#pragma once
#include "dfm_common.h"
#include "dfm_criteria.h"
#include <functional>
#include <vector>

struct dfm_ctx;   // dfm_host.h
struct dfm_ss_mf;   // include/dfm.h
struct dfm_ss_params;
struct dfm_ss_em_out;
struct dfm_ss_em_info;
struct dfm_ss_blocks;

namespace dfm {

// ---- shared types
typedef void (*timer_fn)(void *ctx, int cls, int begin);
struct StatDesc { int kind, arg0, arg1, off; };   // uploaded; indexed by stats_kernel
struct FactBase {   // passed by value into the factored kernels
  int T, r;
  int64_t ldH;
  const double *F, *EL, *S, *H, *cF, *hd;   // T x r, T x r, r x r, T x ldH, T, T
  const double *FtF = nullptr;   // F'F (16 x 16) when the model holds it (else computed per solve)
  // H / hmax in float (T x ldH, zero k-padding), hmax = max_t H[t][t] (H is positive semidefinite: |H32| <= 1), for
  // the fp32 middle products of a warm eigenvalue-rule solve (gemmh_zrm_f32_kernel); nullptr: those stay fp64
  const float *H32 = nullptr;
  double hmax = 0.0;
  // H / hmax as three bf16 planes (hsplit_bytes; launch_fact_hsplit) for the same products as six bf16 terms
  // (gemmh_zrm_split_kernel); nullptr: they run on H32
  const void *Hs = nullptr;
};

// ---- dfm_ctx.hip
int ctx_fail(dfm_ctx *ctx, int code, const char *msg);
hipStream_t ctx_stream(dfm_ctx *ctx);
int ctx_device(dfm_ctx *ctx);

// ---- dfm_gram.hip
hipError_t launch_gram(int orient, const PanelSrc &src, int m, int K, int T, double *G, int64_t ldg,
                       int64_t strideG, int nrep, hipStream_t st);
hipError_t launch_gram_plain_scaled(const double *X, int64_t ld, int m, int K, double *G, int64_t ldg, double alpha,
                                    hipStream_t st);
size_t gram_wk_prep_lds(int T, int r);
int64_t gram_wk_ldk(int N);
int gram_wk_tp(int T);
hipError_t gram_wk_precompute(const double *Ep, int64_t ld, int T, int N, int r, const double *F, const double *L,
                              double *K, double *A0, hipStream_t st);
size_t gram_wk_work(int T, int N, int r, int nb);
double *gram_wk_scratch(double *work, int T, int N, int r, int nb);
hipError_t launch_gram_wk(const double *Ep, int64_t ld, int T, int N, int r, const double *F, const double *L,
                          const double *K, const double *A0, const int32_t *idx, const double *eta, int64_t rs,
                          int nb, double *work, double *G, hipStream_t st);

// ---- dfm_gemm.hip
// Z, the B operand of launch_gemm_zrm / launch_gemm_zrm_f32, replicate-major
// in 16-row chunks: replicate rep's element (s, c) at
// rep zrs + (s >> 4) 16 pz + 16 c + (s & 15), zrs = round_up(T, 16) pz; the
// chunk rows s >= T are zero (the factored solver's boot_prep_kernel writes
// them each call).  The fp32 product's C has the same indexing.
DFM_DEV int64_t zrm_stride(int T, int pz) { return (int64_t)((T + 15) & ~15) * pz; }
DFM_DEV int64_t zrm_ix(int rep, int s, int c, int pz, int64_t zrs) {
  return (int64_t)rep * zrs + (int64_t)(s >> 4) * (16 * pz) + 16 * c + (s & 15);
}
hipError_t launch_gemm_zrm(const double *A, int64_t lda, const double *Z, int pz, int64_t zrs, double *C,
                           int64_t ldc, int M, int Nc, int K, hipStream_t st, const int *col_done, const int *clist,
                           const int *ccount);
hipError_t launch_gemm_zrm_f32(const float *A, int64_t lda, const float *Z, int pz, int64_t zrs, float *C, int M,
                               int Nc, int K, hipStream_t st);
// The bf16-split form of the same product (gemmh_zrm_split_kernel): x ~ h + m + l,
// h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), the differences in fp64,
// each bf16 the round-to-nearest-even of the fp32 rounding (24 significant
// bits in all).  Plane pi = 0, 1, 2 is h, m, l; a 16-B piece holds 8
// consecutive k of one row (H) or column (Z).
//   Hs: piece (k-stage ks, plane pi, k-half kh, row a) at
//       ((ks 3 + pi) 2 + kh) hsplit_rows(T) + a, rows a >= T and k >= T zero;
//   Zs: replicate rep's block starts at byte 8 rep zrs (the fp64 Z's own
//       block), its 16-row chunk ch at byte 96 pz ch, and there piece
//       (pi, kh, column c) is number (2 pi + kh) pz + c; chunk rows >= T zero.
// Two doubles -> one dword of each plane (element 0 in the low half).  The
// fp32 rounding is kept a step of its own (the empty asm: the compiler would
// fold double -> float -> bf16 into one rounding); v_cvt_pk_bf16_f32 rounds to
// nearest even.
DFM_DEV uint32_t bf16_pack2(float a, float b) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  asm volatile("" : "+v"(a), "+v"(b));
  const bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}
DFM_DEV void bf16_split3_pair(double x0, double x1, uint32_t &h, uint32_t &m, uint32_t &l) {
  h = bf16_pack2((float)x0, (float)x1);
  const double r0 = x0 - (double)__uint_as_float(h << 16), r1 = x1 - (double)__uint_as_float(h & 0xFFFF0000u);
  m = bf16_pack2((float)r0, (float)r1);
  const double s0 = r0 - (double)__uint_as_float(m << 16), s1 = r1 - (double)__uint_as_float(m & 0xFFFF0000u);
  l = bf16_pack2((float)s0, (float)s1);
}
// ... and planes h and m alone: the same bits
DFM_DEV void bf16_split2_pair(double x0, double x1, uint32_t &h, uint32_t &m) {
  h = bf16_pack2((float)x0, (float)x1);
  const double r0 = x0 - (double)__uint_as_float(h << 16), r1 = x1 - (double)__uint_as_float(h & 0xFFFF0000u);
  m = bf16_pack2((float)r0, (float)r1);
}
// eight consecutive doubles -> the three planes' 16-B pieces
DFM_DEV void bf16_split3_piece(const double *x, uint4 &ph, uint4 &pm, uint4 &pl) {
  bf16_split3_pair(x[0], x[1], ph.x, pm.x, pl.x);
  bf16_split3_pair(x[2], x[3], ph.y, pm.y, pl.y);
  bf16_split3_pair(x[4], x[5], ph.z, pm.z, pl.z);
  bf16_split3_pair(x[6], x[7], ph.w, pm.w, pl.w);
}
// A wave stores one Z chunk (16 rows x pz columns, column-major doubles st[16 c
// + row], in LDS) as its Zs pieces at dst, the chunk's first piece.  A lane
// splits four doubles and stores each plane's half piece (8 B): twice the
// lanes at half the registers of whole pieces per lane, which the middle
// Horner steps (128 VGPRs) cannot spare.  ONE: 4 pz <= 64, a single round.
// dst must be wave-uniform (the chunk number through readfirstlane): the
// three stores then take a scalar base and one 32-bit lane offset, and no
// 64-bit per-lane address is carried through the caller's tile loop.
// PLANES = 2, for a three-term product: plane l is neither formed nor stored —
// its third of the chunk keeps whatever it held and the product does not
// address it.
template <bool ONE, int PLANES>
DFM_DEV void zsplit_store_chunk(const double *st, int pz, int lane, char *__restrict__ dst) {
  static_assert(PLANES == 2 || PLANES == 3, "planes h, m and perhaps l");
  auto part = [&](int e) {   // e = 4 c + 2 kh + half: doubles 4 e .. 4 e + 3
    uint2 h, m, l;
    if constexpr (PLANES == 3) {
      bf16_split3_pair(st[4 * e], st[4 * e + 1], h.x, m.x, l.x);
      bf16_split3_pair(st[4 * e + 2], st[4 * e + 3], h.y, m.y, l.y);
    } else {
      bf16_split2_pair(st[4 * e], st[4 * e + 1], h.x, m.x);
      bf16_split2_pair(st[4 * e + 2], st[4 * e + 3], h.y, m.y);
    }
    const uint32_t off = 8u * (uint32_t)(2 * (((e >> 1) & 1) * pz + (e >> 2)) + (e & 1));
    *reinterpret_cast<uint2 *>(dst + off) = h;
    *reinterpret_cast<uint2 *>(dst + 32 * pz + off) = m;
    if constexpr (PLANES == 3) *reinterpret_cast<uint2 *>(dst + 64 * pz + off) = l;
  };
  if constexpr (ONE) {
    // (the lane number is re-read here so that the addresses below are formed at the call, from one register: as
    // loop invariants of the caller's tile loop they are carried in five, which the middle steps spill)
    int e = lane;
    asm volatile("" : "+v"(e));
    if (e < 4 * pz) part(e);
  } else {
    for (int e = lane; e < 4 * pz; e += 64) part(e);
  }
}
// ... with the plane count (3 or 2: FilterPlan::z0_planes / mid_planes) a wave-uniform run-time value
template <bool ONE>
DFM_DEV void zsplit_store_chunk(const double *st, int pz, int lane, char *__restrict__ dst, int planes) {
  if (planes == 3) zsplit_store_chunk<ONE, 3>(st, pz, lane, dst);
  else zsplit_store_chunk<ONE, 2>(st, pz, lane, dst);
}
inline int hsplit_rows(int T) { return (T + 127) & ~127; }
inline size_t hsplit_bytes(int T) { return (size_t)((T + 15) / 16) * 6 * hsplit_rows(T) * 16; }
// (terms = 6, or 3: the pairs of planes h and m alone, which read no plane l of either operand)
hipError_t launch_gemm_zrm_split(const void *Hs, const void *Zs, int pz, int64_t zrs, float *C, int M, int Nc, int K,
                                 int terms, hipStream_t st);
// ... and C (M x Nc fp64, row stride ldc, launch_gemm_zrm's layout) = scale C32 from the same kernel's second epilogue
hipError_t launch_gemm_zrm_split_rows(const void *Hs, const void *Zs, int pz, int64_t zrs, double *C, int64_t ldc,
                                      double scale, int M, int Nc, int K, hipStream_t st);
hipError_t launch_gemm_loadings(const double *Eaug, int64_t lda, const double *ZF, int Kp, int rp, int N, int nrep,
                                int K, int r, double invT, double *Lout, hipStream_t st);
int gram_dma_slots(int m);
hipError_t launch_gram_dma(const double *X, int64_t ld, int m, int K, int S, int ksteps, double *G, int64_t ldg,
                           int64_t strideZ, hipStream_t st, double alpha);
hipError_t launch_gemm(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int M,
                       int Nc, int K, hipStream_t st);

// ---- dfm_eig.hip (the explicit-Gram top-k solver)
__global__ void eig_trace_kernel(const double *__restrict__ G, int64_t ldg, int64_t strideG, int m,
                                 double *__restrict__ trace);
const int *eig_iters_ptr(char *ws, int m, int nb, int P, int maxit);
size_t eig_workspace_bytes_padded(int m, int nb, int P, int maxit);
extern thread_local int g_last_iters;   // per host thread: dfm_bootstrap_multi's shards run concurrently
extern thread_local int64_t g_last_rep_iters;
extern thread_local int64_t g_last_gemm_products;
extern thread_local int64_t g_last_gemm_products_f32;   // of those, the fp32 ones (factored solver, host-counted)
extern thread_local int64_t g_last_gemm_products_split_last;   // ... and the warm filter's last products run split
extern thread_local int64_t g_last_gemm_products_split3;       // ... and the fp32 ones run as three bf16 terms
int eig_block_p(int m, int k, int req);
int fact_block_p(int m, int k, int req);
// What both solvers take besides the matrix.  Callers fill the members by name.
struct EigArgs {
  int nb, k, p;                   // problems, wanted pairs, block columns (k <= p <= 32)
  const double *warm;             // m x kw start vectors shared by all problems (nullptr, 0: hashed start)
  int kw;
  double tol;                     // >= 0: eigenvector residual rule; < 0: eigenvalue bound
  int maxit, poll;
  char *ws;                       // eig_workspace_bytes_padded
  double *lam, *Uk, *trace_out;   // nb x k, nb x m x k (nullptr: eigenvalues only), nb
  int *status;                    // nb
  hipStream_t st;
  timer_fn tf;
  void *tctx;
  int subspace = 0;               // EigWork::subspace
  int fused = -1;                 // the one-workgroup solver (m <= 256, P = 16): -1 as DFM_EIG_FUSED says, 0 off, 1 on
};
int eig_run(const double *G, int64_t ldg, int64_t strideG, int m, const EigArgs &a, int *iters_host, int64_t rep0);

// ---- dfm_fact.hip (the factored bootstrap solver)
size_t fact_workspace_bytes(int T, int nb, int P);
// What the factored solver takes on top of EigArgs.
struct FactArgs {
  const int32_t *idx;             // nb x T draws
  const double *eta;
  char *fws;                      // fact_workspace_bytes
  int *off, *lst;                 // the draws' CSR (out; fact_loadings reads it)
  long long *cnt = nullptr;       // device counters of replicate-iterations and GEMM products (nullptr: host stats)
  double spread = 0.0;            // lambda_1 / lambda_k of the base fit (>= 1: warm schedule)
  double lamk = 0.0;              // lambda_k of the base fit (> 0: a warm solve may start with the filter)
  double fscale = 0.0;            // s > 0: fb.F = s * warm[:, :r], one rounding per element (0: no such identity)
  const PollBuf *pb = nullptr;
};
int eig_run_factored(const FactBase &fb, const EigArgs &a, const FactArgs &f);
int fact_t_max();
hipError_t launch_fact_ftf(const FactBase &fb, double *FtF, hipStream_t st);

// ---- dfm_fact_model.hip (model-level factored precompute, explicit factored Gram, loadings)
int fact_loadings(const FactBase &fb, const double *Ep, int64_t ld, int N, const double *Lb,
                  const double *Uk, const double *eta, const int *off, const int *lst, int nb,
                  double *Fout, double *Lout, char *ws, hipStream_t st);
size_t fact_loadings_bytes(int T, int N, int r, int nb);
hipError_t launch_fact_fsf(int T, int r, const double *Fb, const double *S, double *FSF, int64_t ldH, hipStream_t st);
hipError_t launch_gram_fact(const FactBase &fb, const double *FSF, const int32_t *idx, const double *eta, int nb,
                            double *G, int64_t ldg, int64_t strideG, hipStream_t st);
int fact_precompute(const double *Ep, int64_t ld, int T, int N, int r, const double *Lb, const double *Fb,
                    const double *H, int64_t ldH, double *EL, double *S, double *cF, double *hd, hipStream_t st);
hipError_t launch_fact_h32(const double *H, int64_t ldH, int T, const double *hd, float *H32, hipStream_t st);
hipError_t launch_fact_hsplit(const double *H, int64_t ldH, int T, const double *hd, void *Hs, hipStream_t st);
double fact_hmax(const double *hd_host, int T);

// ---- dfm_model.hip
__global__ void panel_from_colmajor_kernel(const double *__restrict__ X, int64_t ldx, int T, int N,
                                           double *__restrict__ P, int64_t ld);
__global__ void colmajor_from_rows_kernel(const double *__restrict__ P, int64_t ld, int T, int N,
                                          double *__restrict__ X);
__global__ void colssr_cols_kernel(const double *__restrict__ G, int64_t ldg, int64_t strideG, int N,
                                   int k, const double *__restrict__ lam,
                                   const double *__restrict__ Uk, double *__restrict__ colssr);
__global__ void common_residual_kernel(const double *__restrict__ X, int64_t ld, int T, int N, int k,
                                       const double *__restrict__ F, const double *__restrict__ L,
                                       double *__restrict__ C, double *__restrict__ E);
__global__ void panel_row_ssq_kernel(const double *__restrict__ E, int64_t ld, int T,
                                     double *__restrict__ rows);
__global__ void ordered_sum_kernel(const double *__restrict__ v, int n, double *__restrict__ out);
hipError_t launch_ols(int nb, hipStream_t st, const double *y, const double *w, int q, const double *F, int Tphys,
                      int kF, const int *Tn, const int *kr, double *coef, double *tstat, double *cov_out,
                      double *resid_out, int *status, const int *R0 = nullptr);
__global__ void tail_sigma2_kernel(const double *__restrict__ ev, int m, int nb, double NT,
                                   double *__restrict__ sig2);
__global__ void stats_kernel(int nb, int T, int N, int r, int q, int crit, double sigma2,
                             const double *__restrict__ sig2v,
                             const double *__restrict__ lam, const double *__restrict__ trace,
                             const double *__restrict__ coef, const double *__restrict__ tstat,
                             const int *__restrict__ iters, const StatDesc *__restrict__ sd, int ns,
                             double *__restrict__ out, int64_t width, const int *__restrict__ st1,
                             const int *__restrict__ st2, int *__restrict__ flag);
int launch_factors(int orient, const PanelSrc &src, int T, int N, int k, int nb,
                   const double *Uk, double *F, double *L, double *colssr, hipStream_t st,
                   double Ts = 0, int64_t fstride = 0);
bool launch_factors_cols_fact(const double *Ep, int64_t ld, int T, int N, int k, const double *Fb, const double *Lb,
                              int rb, const int32_t *idx, const double *eta, int64_t rs, int nb, const double *Uk,
                              double *F, double *L, int64_t fstride, double *G, hipStream_t st);
__global__ void col_ssq_kernel(const double *__restrict__ E, int64_t ld, int T, int N,
                               double *__restrict__ out);
__global__ void block_accum_kernel(const double *__restrict__ lam_b, const double *__restrict__ tr_b,
                                   int nb, int r, double *__restrict__ lam, double *__restrict__ tr,
                                   int first);

// ---- dfm_chow.hip
size_t chow_workspace_bytes(int T, int N, int r, int nb);
hipError_t launch_chow(int orient, const PanelSrc &src, int T, int N, int r, int bp, int nb,
                       const double *F, const double *Lm, double *LRo, double *LMo, double *WDo,
                       int64_t out_stride, char *ws, size_t ws_bytes, hipStream_t st, int nblk = 1,
                       const int *brow = nullptr, int64_t lbs = 0);
size_t targeted_workspace_bytes(int mode, int T, int N, int q);
hipError_t launch_targeted(int mode, const double *y, const double *w, int q, const double *Xp,
                           int64_t ld, int T, int N, double cv, double *tstat, uint8_t *mask, char *ws,
                           size_t ws_bytes, hipStream_t st, int *bad);

// ---- dfm_chow_sweep.hip (every break period bp_lo..bp_hi at once; r <= 16, no breaks)
// Outputs of a sweep (device pointers; any may be nullptr, index 0 / 1 / 2 =
// LR / LM / Wald): sup[s] + rep * os + i, argsup[s] (nb x N break periods),
// curve[s] (nb x nbp x N).  A statistic none of whose outputs is set is not computed.
struct ChowSweepOut {
  double *sup[3] = {nullptr, nullptr, nullptr};
  int64_t os = 0;
  int64_t *argsup[3] = {nullptr, nullptr, nullptr};
  double *curve[3] = {nullptr, nullptr, nullptr};
};
size_t chow_sweep_workspace_bytes(int T, int N, int r, int nbp, int nb);
hipError_t launch_chow_sweep(const PanelSrc &src, int T, int N, int r, int bp_lo, int bp_hi, int nb, const double *F,
                             const double *Lm, const ChowSweepOut &out, char *ws, size_t ws_bytes, hipStream_t st,
                             timer_fn tf = nullptr, void *tctx = nullptr);

// ---- dfm_spec.hip
int spectrum_max();
int64_t spectrum_work(int m, int nb);
int spectrum_any_max();
hipError_t launch_spectrum_var(const double *G, int64_t ldg, int64_t strideG, int m, int m0, int dm, int nb,
                               double *ev, double *work, hipStream_t st);
hipError_t launch_spectrum(const double *G, int64_t ldg, int64_t strideG, int m, int nb, double *ev,
                           double *work, hipStream_t st);
int dense_eig_max();
int64_t dense_eig_work(int m, int k);
hipError_t launch_dense_eig_batched(const double *G, int64_t ldg, int64_t strideG, int m, int mv0, int dmv, int nb,
                                    int k, double *lam, double *Uk, double *trace, int *status, double *work,
                                    hipStream_t st);
hipError_t launch_dense_eig(const double *G, int64_t ldg, int m, int k, double *lam, double *Uk, double *trace,
                            int *status, double *work, hipStream_t st);

// ---- dfm_wide.hip
hipError_t gemm_batched(int nb, int M, int Nc, int K, double alpha, const double *A, int64_t sAr, int64_t sAc,
                        int64_t sAb, const double *B, int64_t sBr, int64_t sBc, int64_t sBb, double beta, double *C,
                        int64_t sCr, int64_t sCc, int64_t sCb, hipStream_t st);
hipError_t launch_materialize(const PanelSrc &src, int T, int N, int64_t ld, int nb, double *X, hipStream_t st);
int launch_factors_wide(int orient, const double *X, int64_t ld, int T, int N, int k, const double *Uk,
                        double *F, double *L, double *colssr, hipStream_t st, double Ts, int nb = 1, int64_t sX = 0,
                        int64_t fstride = 0);
int64_t ols_wide_work(int T, int d);
hipError_t launch_ols_wide_batched(int nb, const double *y, const double *w, int q, const double *F, int T, int kF,
                                   int k, const int *Tn, double *coef, double *tstat, double *cov_out,
                                   double *resid_out, int *status, double *work, hipStream_t st, int hc0 = 0);
hipError_t launch_ols_wide(const double *y, const double *w, int q, const double *F, int T, int k, double *coef,
                           double *tstat, double *cov_out, double *resid_out, int *status, double *work,
                           hipStream_t st);
hipError_t launch_targeted_joint_wide(const double *y, const double *w, int q, const double *X, int64_t ld, int T,
                                      int N, double cv, double *tx, uint8_t *mask, int *status, double *work,
                                      hipStream_t st);
int64_t targeted_joint_wide_work(int T, int q, int N, int64_t ld);
int64_t chow_wide_work(int T, int N, int r);
hipError_t launch_chow_wide(int nb, const double *X, int64_t ld, int64_t sX, const double *E, int T, int N, int r,
                            int bp, const double *F, int64_t sF, const double *L, int64_t sL, double *LR, double *LM,
                            double *WD, int64_t ostr, double *scr, double *work, hipStream_t st, int nblk = 1,
                            const int *brow = nullptr, int64_t lbs = 0);

// ---- dfm_predict.hip
hipError_t launch_predict(const double *Xp, int64_t ld, int T, int N, const double *L, int r, const double *x_dev,
                          int64_t ldx, int64_t nn, const double *w_dev, int64_t ldw, int q, const double *beta_dev,
                          double *work, double *F_out, double *yhat, hipStream_t st);

// ---- dfm_ss.hip
constexpr int SS_LS = 33, SS_MAT = 32 * SS_LS;   // row stride and size of an LDS matrix (s <= 32)
// C_t's lower triangle in a collapsed row: element (i, j) at column i (i + 1) / 2 + j.
__host__ __device__ inline int ss_tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }
constexpr int SS_KC = 256;                    // panel columns per K chunk (a multiple of 16)
DFM_DEV int ss_offA(int a, int kc) { return a * 16 + (kc ^ (((a >> 1) & 1) << 3)); }   // [a][k]
DFM_DEV int ss_offB(int a, int kc) { return kc * 64 + (a ^ ((kc & 7) << 2)); }         // [k][a]
// Columns of a collapsed row: C_t's lower triangle (ss_tri), b_t, q_t, n_t, l_t.
inline int ss_ncols(int r) { return r * (r + 1) / 2 + r + 3; }
// The smoother's moments of a panel (ss_smoother_kernel<true>): S11, S10, S00, a_1|T, P_1|T at SS_M*.
constexpr int SS_M11 = 0, SS_M10 = 256, SS_M00 = 768, SS_MA1 = 1792, SS_MP1 = 1824, SS_MOM = 2848;
struct SsParams {   // checked, host
  int r = 0, p = 0;
  const double *L = nullptr, *sigma2 = nullptr, *A = nullptr, *Q = nullptr, *a0 = nullptr, *P0 = nullptr;
};
// The launch geometry of a pass over panels of one shape, stated once (ss_geom).
// mixed: the mixed-frequency model, whose collapsed row holds a tri(C) | b
// group per class and the low class's count after l_t.
// ar: AR(1) idiosyncratic terms, whose collapsed row is the plain one at the
// update's size ru = 2r (ru = r otherwise).
struct SsGeom {
  int T, Tt, N, r, s;              // Tt = T + horizon rows, s the state
  bool mixed, ar;
  int ru;                          // the size of the update block
  int cq, ncols, nct, NCP, Npad;   // q_t's column, a collapsed row's columns, their 64-wide tiles and 64 nct; N to 16
  int nrt, Tpad, KS;               // the collapse: 64-row tiles, 64 nrt, K chunks of SS_KC columns
  int nrn, Nr, KT;                 // the M-step (its transpose): 64-series tiles, 64 nrn, K chunks of SS_KC rows
};
SsGeom ss_geom(int T, int h, int N, int r, int s, bool mixed, bool ar = false);
// Panel b's parameter block (ss_block), as the kernels address it.  With AR(1)
// terms Wm, Wv are the pair entries' operands, Wsm, Wsv the start entries' and
// rho follows winv (all three absent otherwise).
struct SsBlock {
  int64_t stride, oWm, oWv, oWsm, oWsv, owi, orho, oTm, oQ, oa0, oP0, oL, osig;
};
SsBlock ss_block(const SsGeom &G);
int ss_fill_block(const SsParams &pr, const SsGeom &G, const SsBlock &B, double *hp, const uint8_t *low = nullptr,
                  const double *rho = nullptr);
// What a one-panel ss_smooth_core call holds when its launches are done and
// checked, handed to `after` before it is freed: the geometry they ran at, the
// collapsed rows, the recursion's workspace, and the parameters on both sides
// of the bus.
struct SsKept {
  SsGeom g;
  const double *part, *ws;                 // device: [chunk][Tpad][NCP]; a_t|t, a_t|t-1, P_t|t, P_t|t-1
  const double *dTm, *dP0;                 // device, row-major s x s
  const double *hTm, *hQ, *ha0, *hP0;      // host, row-major (Q r x r, a0 s)
};
struct SsAfter {
  virtual int run(const SsKept &k) = 0;
  virtual ~SsAfter() = default;
};
int ss_param_error(dfm_ctx *ctx, const char *who, int rc, int64_t where);
// The same for the entry points with AR(1) idiosyncratic terms: their limits,
// and -2 with `where` >= 0 names the column of rho that is not inside (-1, 1).
int ss_ar_error(dfm_ctx *ctx, const char *who, int rc, int64_t where);
int ss_smooth_core(dfm_ctx *ctx, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx, int64_t stride,
                   bool dev, const SsParams &pr, int h, double *filt, double *smooth, double *cov, double *loglik,
                   int64_t *nobs, const dfm_ss_mf *mf = nullptr, double *agg = nullptr, SsAfter *after = nullptr,
                   const char *who_plain = "dfm_ss_smooth", const double *rho = nullptr);
// One device block from the stream's pool, freed on the stream on every return path.
struct StreamBuf {
  void *p = nullptr;
  hipStream_t st = nullptr;
  ~StreamBuf() {
    if (p) hipFreeAsync(p, st);
  }
  hipError_t alloc(size_t bytes, hipStream_t s) {
    st = s;
    return stream_malloc(&p, bytes > 8 ? bytes : 8, s);
  }
};
// The panels of a pass where the kernels read them: a device batch in place, a
// host batch through one device buffer of the largest pass's span.
struct SsStage {
  const double *X;
  int64_t ldx, stride;
  int T, N;
  bool dev;
  hipStream_t st;
  StreamBuf dx;
  int64_t span(int64_t n) const { return (n - 1) * stride + ldx * (int64_t)(N - 1) + T; }
  hipError_t alloc(int64_t mb) { return dev ? hipSuccess : dx.alloc((size_t)span(mb) * 8, st); }
  hipError_t pass(int64_t c0, int64_t n, const double **src) {   // panels c0 .. c0 + n - 1
    *src = X + c0 * stride;
    if (dev) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dx.p, *src, (size_t)span(n) * 8, hipMemcpyHostToDevice, st);
    *src = (const double *)dx.p;
    return e;
  }
};
// One E-step over the n panels of a pass (ss_estep): the collapse, then the
// filter and the smoother.
struct SsEstep {
  const double *X;                           // the staged panels (SsStage::pass) and their layout
  int64_t ldx, stride;
  const double *par;                         // the parameter block of the pass's first panel (device) and the
  int64_t pstride;                           // panel stride of the blocks (0: every panel reads that one)
  const int *active;                         // null, or per panel: 0 = frozen
  double *part, *ws;                         // the collapsed rows and the recursion's workspace
  double *filt, *smooth, *cov, *ll, *nobs;   // per panel T x r, Tt x r, Tt x r x r, 1, 1 (nullptr: not wanted)
  int *flag;                                 // per panel, for ss_estep_error
  double *opnd, *mom;                        // given: the smoother also leaves the M-step's operand rows and moments
  int nw;                                    // mixed frequency: the weights (device) and the smoothed aggregate
  const double *w;
  double *agg;
};
int ss_estep(dfm_ctx *ctx, const SsGeom &G, const SsBlock &B, const SsEstep &e, int64_t n);
// A panel's non-zero E-step flag as SS_E_SINGULAR; iteration >= 0: the EM's.
int ss_estep_error(dfm_ctx *ctx, const char *who, long long panel, int flag, int iteration = -1);
// The mixed-frequency arguments of the entry point `who`, in the order and the
// words all three refuse them.  *lags: 0 when no series is marked (the caller
// runs the plain entry point), else the state's lags max(p, n_w).  rest_ok:
// the caller's own arguments, refused after the mask and before the weights
// (r and p are read only when it holds); dims names what the weights' message
// asks to be >= 1.
int ss_mf_args(dfm_ctx *ctx, const char *who, const dfm_ss_mf *mf, int64_t N, bool rest_ok, int r, int p,
               const char *dims, int *lags);
// The padded state's copies of n parameter sets of one (r, p): p = L and A =
// [A 0] (held by Apad).  -1, or the first set with another (r, p) or no A.
int64_t ss_mf_pad_params(const dfm_ss_params *sets, int64_t n, int r, int p, int L, std::vector<dfm_ss_params> &padded,
                         std::vector<double> &Apad);

// ---- dfm_ss_lane.hip
// What follows a one-panel smooth in dfm_ss_simulate and dfm_ss_news (their
// SsAfter::run): ss_gain_kernel once, one record per row (dfm_ss_lane.h), then
// the feature's lane kernel over its columns (draws, releases) in passes, a
// wave of 64 columns per workgroup.  A job states the feature's side.
struct SsLaneJob {
  bool sim;                  // the record carries b_t and R_t
  int nw, w_at;              // the mixed model's weights: their count and where they start in cst
  std::vector<double> cst;   // the lane kernel's constants (host; the driver uploads them)
  const void *kernel;        // the lane kernel; it takes one struct by value
  void *args;                // that struct, on the host: the inputs callback must assign it before it returns
  size_t lds;                // the kernel's dynamic LDS bytes (beyond 64 KB the driver raises the kernel's cap)
  int64_t count, per_pass;   // the columns, and how many a pass takes
  size_t per_out;            // doubles of a column in one output plane
  int planes;                // output planes a lane writes, one after the other ([per_out][n] each)
  double *host[2];           // where plane q leaves for ([count][per_out]; null: not wanted)
};
struct SsLaneBufs {
  const double *cst, *rec;   // the constants and the records on the device
  double *cf, *out;          // the pass's c_t|t [Tt][s][n] and its planes
  hipStream_t st;
};
// Columns c0 .. c0 + n - 1: stage what the lane kernel reads of them, then assign *job.args (the driver launches
// job.kernel with it as soon as this returns); non-zero: the error.
using SsLaneInputs = std::function<int(int64_t c0, int64_t n, const SsLaneBufs &b)>;
// Per pass: inputs, the lane kernel (DFM_KC_FACTORS), the wanted planes
// transposed to [column][per_out] (DFM_KC_GEMM) and copied out, one stream
// synchronise.  The gains report as DFM_KC_OLS.
int ss_lane_run(dfm_ctx *ctx, const SsKept &k, const SsLaneJob &job, const SsLaneInputs &inputs);

// ---- dfm_ss_em.hip
// mf: the mixed-frequency model (checked): the starts are then the padded
// state's (p = max(p_var, n_w), A = [A 0]), p_var the VAR's own lag count
// (out.A is r x r p_var); null: the plain model.
// blocks: the factor blocks (checked, the starts too: dfm_ss_em_blocks); null:
// no restriction.
struct SsBlockOff {   // the kernels' view: block g owns the factors off[g] .. off[g + 1] - 1
  int nb;
  uint8_t off[17];
};
struct SsBlocks {
  SsBlockOff o;
  const uint16_t *free;   // host, N: bit j set when the series loads on factor j
};
int ss_em_core(dfm_ctx *ctx, const char *who, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx,
               int64_t stride, bool dev, const dfm_ss_params *starts, int64_t n_start, int max_iter, double tol,
               bool update_init, int h, const dfm_ss_em_out &out, dfm_ss_em_info *info, const dfm_ss_mf *mf = nullptr,
               int p_var = 0, const SsBlocks *blocks = nullptr);
// The checked blocks of the entry point `who` (r = the sum the sizes must have):
// 0 with *trivial set when there is no restriction, else with bl and the mask
// it points to filled; -2 / -7 with the message otherwise.
int ss_blocks_args(dfm_ctx *ctx, const char *who, const dfm_ss_blocks *blocks, int64_t N, int r, bool *trivial,
                   SsBlocks *bl, std::vector<uint16_t> &free);

}  // namespace dfm
