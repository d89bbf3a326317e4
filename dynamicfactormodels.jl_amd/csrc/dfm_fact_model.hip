// dfm_fact_model.hip — the factored bootstrap's model-level side: what a model
// precomputes once for the factored solver of dfm_fact.hip (fact_precompute:
// EL, S, cF, diag H), the replicates' loadings after a solve (fact_loadings)
// and the explicit replicate Grams formed from the same factors
// (launch_fact_fsf, launch_gram_fact).
#include "dfm_internal.h"
#include <algorithm>

namespace dfm {

// ---- factored loadings pass: L* = X*' F* / T = (L (F'F*) + E' P' D F*) / T
// boot_zf: replicate rep's block ZB = ZF + rep Kp rp (Kp x rp, row-major):
//          ZB[s][j] = sum_{t in bucket s} eta_t F*[t][j]   (s < T)
//          ZB[T + i][j] = M1[rep][i][j] = (F' F*)[i][j]    (i < r)
//          zero rows T + r .. Kp - 1 and zero column r when rp > r;
//          F* = sqrt(T) U* written to Fout.
// The block is contiguous, so every row segment lands in whole lines.
__global__ __launch_bounds__(256) void boot_zf_kernel(FactBase fb, const double *__restrict__ Uk,
                                                      const double *__restrict__ eta,
                                                      const int *__restrict__ off, const int *__restrict__ lst,
                                                      double *__restrict__ Fout, double *__restrict__ ZF, int Kp,
                                                      int rp, double *__restrict__ M1) {
  const int tid = threadIdx.x, rep = blockIdx.x, T = fb.T, r = fb.r;
  const double sT = sqrt((double)T);
  const double *U = Uk + (int64_t)rep * T * r;
  double *Fr = Fout + (int64_t)rep * T * r;
  double *ZB = ZF + (int64_t)rep * Kp * rp;
  const double *et = eta ? eta + (int64_t)rep * T : nullptr;
  const int *o = off + (int64_t)rep * (T + 1);
  const int *L = lst + (int64_t)rep * T;
  for (int e = tid; e < T * r; e += 256) Fr[e] = sT * U[e];
  for (int e = tid; e < T * rp; e += 256) {
    const int sI = e / rp, j = e - sI * rp;
    double z = 0.0;
    if (j < r)
      for (int q = o[sI]; q < o[sI + 1]; ++q) {
        const int t = L[q];
        z = fma(et ? et[t] : 1.0, sT * U[(int64_t)t * r + j], z);
      }
    ZB[e] = z;
  }
  for (int e = (T + r) * rp + tid; e < Kp * rp; e += 256) ZB[e] = 0.0;
  if (rp > r)
    for (int i = tid; i < r; i += 256) ZB[(int64_t)(T + i) * rp + r] = 0.0;
  // M1 = F' F*: 4 row-interleaved partial sums per entry (four independent
  // chains of T/4 instead of one of T), combined in a fixed order
  __shared__ double m1p[4][256];
  const int part = tid >> 6;
  for (int e0 = 0; e0 < r * r; e0 += 64) {
    const int e = e0 + (tid & 63);
    double acc = 0.0;
    if (e < r * r) {
      const int i = e / r, j = e % r;
      for (int t = part; t < T; t += 4) acc = fma(fb.F[(int64_t)t * r + i], sT * U[(int64_t)t * r + j], acc);
    }
    m1p[part][tid & 63] = acc;
    __syncthreads();
    if (tid < 64 && e < r * r) {
      const double v = (m1p[0][tid] + m1p[1][tid]) + (m1p[2][tid] + m1p[3][tid]);
      M1[(int64_t)rep * r * r + e] = v;
      // the same block as k-rows T..T+r-1 of the loadings GEMM's B operand
      ZB[(int64_t)(T + e / r) * rp + e % r] = v;
    }
    __syncthreads();
  }
}

// rows T.. of [E; L'; 0]: row T+i = column i of L (i < r), then zero rows
__global__ void eaug_tail_kernel(const double *__restrict__ Lb, int N, int r, int64_t ld, double *__restrict__ tail) {
  const int i = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= ld) return;
  tail[(int64_t)i * ld + n] = (i < r && n < N) ? Lb[n * r + i] : 0.0;
}

static int zf_rp(int r) { return (r + 1) / 2 * 2; }
static int zf_kp(int T, int r) { return (T + r + 15) / 16 * 16; }
int fact_loadings(const FactBase &fb, const double *Ep, int64_t ld, int N, const double *Lb,
                  const double *Uk, const double *eta, const int *off, const int *lst, int nb,
                  double *Fout, double *Lout, char *ws, hipStream_t st) {
  const int T = fb.T, r = fb.r, rp = zf_rp(r), Kp = zf_kp(T, r);
  double *ZF = (double *)ws;                       // nb blocks of Kp x rp
  double *M1 = ZF + (size_t)nb * Kp * rp;
  double *Eaug = M1 + (size_t)nb * r * r;          // [E; L'; 0]: Kp x ld
  // (staging U*, eta and the CSR in LDS first measured slower: 0.62 -> 0.76 ms at C3)
  hipLaunchKernelGGL(boot_zf_kernel, dim3(nb), dim3(256), 0, st, fb, Uk, eta, off, lst, Fout, ZF, Kp, rp, M1);
  // one GEMM of depth T + r does the whole finish (see gemm_loadings_kernel),
  // for every batch size: the same arithmetic for every replicate whatever
  // the batch composition (batch- and shard-invariant loadings)
  hipMemcpy2DAsync(Eaug, (size_t)ld * 8, Ep, (size_t)ld * 8, (size_t)ld * 8, T, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(eaug_tail_kernel, dim3((unsigned)((ld + 255) / 256), Kp - T), dim3(256), 0, st, Lb, N, r, ld,
                     Eaug + (size_t)T * ld);
  const hipError_t e = launch_gemm_loadings(Eaug, ld, ZF, Kp, rp, N, nb, T + r, r, 1.0 / T, Lout, st);
  return e == hipSuccess ? 0 : 1000 + (int)e;
}
size_t fact_loadings_bytes(int T, int N, int r, int nb) {
  const int64_t ld = ((int64_t)N + 15) / 16 * 16;
  const int Kp = zf_kp(T, r);
  return ((size_t)nb * Kp * zf_rp(r) + (size_t)nb * r * r + (size_t)Kp * ld) * 8 + 1024;
}

// ---- model-level precompute: EL = E L (T x r), S = L'L, cF, hd
__global__ void fact_pre_kernel(const double *__restrict__ Ep, int64_t ld, int T, int N, int r,
                                const double *__restrict__ Lb, const double *__restrict__ Fb,
                                const double *__restrict__ H, int64_t ldH, double *__restrict__ EL,
                                double *__restrict__ S, double *__restrict__ cF, double *__restrict__ hd) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < r * r) {
    const int i = threadIdx.x / r, j = threadIdx.x % r;
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc = fma(Lb[(int64_t)n * r + i], Lb[(int64_t)n * r + j], acc);
    S[threadIdx.x] = acc;
  }
  if (t >= T) return;
  for (int j = 0; j < r; ++j) {
    double acc = 0.0;
    for (int n = lane; n < N; n += 64) acc = fma(Ep[(int64_t)t * ld + n], Lb[(int64_t)n * r + j], acc);
    acc = wave_sum(acc);
    if (lane == 0) EL[(int64_t)t * r + j] = acc;
  }
  if (lane == 0) hd[t] = H[(int64_t)t * ldH + t];
}
__global__ void fact_cf_kernel(int T, int r, const double *__restrict__ Fb, const double *__restrict__ S,
                               double *__restrict__ cF) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  double acc = 0.0;
  for (int i = 0; i < r; ++i) {
    double u = 0.0;
    for (int j = 0; j < r; ++j) u = fma(S[i * r + j], Fb[(int64_t)t * r + j], u);
    acc = fma(Fb[(int64_t)t * r + i], u, acc);
  }
  cF[t] = acc;
}
// FSF = F S F' (T x T, ldH), the common-component Gram C C' of the base fit
// (C = F L', S = L'L): entry (s, t >= s) computed once and mirrored, so the
// matrix is exactly symmetric.
__global__ void fact_fsf_kernel(int T, int r, const double *__restrict__ Fb, const double *__restrict__ S,
                                double *__restrict__ FSF, int64_t ldH) {
  const int t = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (t >= T || t < s) return;
  double acc = 0.0;
  for (int i = 0; i < r; ++i) {
    double u = 0.0;
    for (int j = 0; j < r; ++j) u = fma(S[i * r + j], Fb[(int64_t)t * r + j], u);
    acc = fma(Fb[(int64_t)s * r + i], u, acc);
  }
  FSF[(int64_t)s * ldH + t] = acc;
  FSF[(int64_t)t * ldH + s] = acc;
}
hipError_t launch_fact_fsf(int T, int r, const double *Fb, const double *S, double *FSF, int64_t ldH, hipStream_t st) {
  hipLaunchKernelGGL(fact_fsf_kernel, dim3((T + 255) / 256, T), dim3(256), 0, st, T, r, Fb, S, FSF, ldH);
  return hipGetLastError();
}

// Replicate Grams of the direct (Gram-forming) path for N > T without
// breaks, by the factored identity instead of the T x T x N SYRK:
//   X* = F L' + D P E  =>  G* = X* X*' = F S F' + F c' + c F' + D P H P' D,
//   c_t = eta_t EL[idx_t]  (EL = E L, H = E E', S = L'L: model precompute),
// i.e. G*[s][t] = FSF[s][t] + sum_j (F_sj c_tj + c_sj F_tj)
//                 + (eta_s eta_t) H[idx_s][idx_t]          (2 T^2 r flop, not T^2 N).
// Each term is symmetric in (s, t) operation by operation (separately rounded
// products and sums — no contraction — in a fixed order), so G* is exactly
// symmetric.
// One workgroup per (replicate, GF_R rows): the rows' H rows H[idx_s][:]
// staged in LDS (gathered by idx_t from there), one thread per column t
// holding F_t and c_t in registers.
constexpr int GF_R = 8;
template <int RM>
__global__ __launch_bounds__(256) void gram_fact_kernel(FactBase fb, const double *__restrict__ FSF,
                                                        const int32_t *__restrict__ idx,
                                                        const double *__restrict__ eta, int R,
                                                        double *__restrict__ G, int64_t ldg, int64_t strideG) {
  extern __shared__ double gdyn[];
  const int T = fb.T, r = fb.r, tid = threadIdx.x, rep = blockIdx.y, s0 = blockIdx.x * R;
  const int ns = min(R, T - s0);
  double *sH = gdyn;                       // R x T: H[idx_s][:]
  double *sFc = sH + (size_t)R * T;        // R x 2 RM: F_s, c_s
  const int32_t *ix = idx + (int64_t)rep * T;
  const double *et = eta ? eta + (int64_t)rep * T : nullptr;
  for (int e = tid; e < ns * T; e += 256) {
    const int i = e / T, t = e - i * T;
    sH[e] = fb.H[(int64_t)ix[s0 + i] * fb.ldH + t];
  }
  for (int e = tid; e < ns * RM; e += 256) {
    const int i = e / RM, j = e - i * RM, sI = s0 + i;
    const double es = et ? et[sI] : 1.0;
    sFc[i * 2 * RM + j] = j < r ? fb.F[(int64_t)sI * r + j] : 0.0;
    sFc[i * 2 * RM + RM + j] = j < r ? es * fb.EL[(int64_t)ix[sI] * r + j] : 0.0;
  }
  __syncthreads();
  double *Gr = G + (int64_t)rep * strideG;
  for (int t = tid; t < T; t += 256) {
    const int it = ix[t];
    const double eT = et ? et[t] : 1.0;
    double Ft[RM], ct[RM];
#pragma unroll
    for (int j = 0; j < RM; ++j) {
      Ft[j] = j < r ? fb.F[(int64_t)t * r + j] : 0.0;
      ct[j] = j < r ? eT * fb.EL[(int64_t)it * r + j] : 0.0;
    }
    // GF_R rows at a time: every row's FSF entry and H gather issued before the sums
    for (int i0 = 0; i0 < ns; i0 += GF_R) {
      double fsf[GF_R], hv[GF_R], es[GF_R];
#pragma unroll
      for (int u = 0; u < GF_R; ++u) {
        const int i = min(i0 + u, ns - 1), sI = s0 + i;
        fsf[u] = FSF[(int64_t)sI * fb.ldH + t];
        hv[u] = sH[i * T + it];
        es[u] = et ? et[sI] : 1.0;
      }
#pragma unroll
      for (int u = 0; u < GF_R; ++u) {
        const int i = i0 + u;
        if (i >= ns) break;
        const double *fc = sFc + i * 2 * RM;
        double x = 0.0;
#pragma unroll
        for (int j = 0; j < RM; ++j)
          if (j < r) x = __dadd_rn(x, __dadd_rn(__dmul_rn(fc[j], ct[j]), __dmul_rn(fc[RM + j], Ft[j])));
        Gr[(int64_t)(s0 + i) * ldg + t] = __dadd_rn(__dadd_rn(fsf[u], x), __dmul_rn(__dmul_rn(es[u], eT), hv[u]));
      }
    }
  }
}
int gram_fact_rows(int T) { return std::max(1, std::min(GF_R, 4096 / std::max(T, 1))); }
size_t gram_fact_lds(int T, int r) {
  const int R = gram_fact_rows(T), RM = r <= 8 ? 8 : 16;
  return (size_t)R * T * 8 + (size_t)R * 2 * RM * 8;
}
hipError_t launch_gram_fact(const FactBase &fb, const double *FSF, const int32_t *idx, const double *eta, int nb,
                            double *G, int64_t ldg, int64_t strideG, hipStream_t st) {
  const int R = gram_fact_rows(fb.T);
  const size_t lds = gram_fact_lds(fb.T, fb.r);
  dim3 grid((fb.T + R - 1) / R, nb);
  if (fb.r <= 8)
    hipLaunchKernelGGL(gram_fact_kernel<8>, grid, dim3(256), lds, st, fb, FSF, idx, eta, R, G, ldg, strideG);
  else
    hipLaunchKernelGGL(gram_fact_kernel<16>, grid, dim3(256), lds, st, fb, FSF, idx, eta, R, G, ldg, strideG);
  return hipGetLastError();
}

// H32 = float(H / hmax), hmax = max_t H[t][t] (fact_hmax: the same number on
// the host, the max being exact in any order): the fp32 H.Z GEMM's left
// operand (gemmh_zrm_f32_kernel), a constant of the fit.  H = E E' is
// positive semidefinite, so |H[s][t]| <= hmax and |H32| <= 1 whatever the
// panel's scale; H's zero k-padding columns stay zero.  One workgroup per row.
__global__ __launch_bounds__(256) void fact_h32_kernel(const double *__restrict__ H, int64_t ldH, int T,
                                                       const double *__restrict__ hd, float *__restrict__ H32) {
  __shared__ double red[256];
  const int tid = threadIdx.x, t = blockIdx.x;
  double mx = 0.0;
  for (int s = tid; s < T; s += 256) mx = fmax(mx, hd[s]);
  red[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmax(red[tid], red[tid + o]); __syncthreads(); }
  const double hmax = red[0] > 0.0 ? red[0] : 1.0;
  for (int64_t c = tid; c < ldH; c += 256) H32[(int64_t)t * ldH + c] = (float)(H[(int64_t)t * ldH + c] / hmax);
}
hipError_t launch_fact_h32(const double *H, int64_t ldH, int T, const double *hd, float *H32, hipStream_t st) {
  hipLaunchKernelGGL(fact_h32_kernel, dim3(T), dim3(256), 0, st, H, ldH, T, hd, H32);
  return hipGetLastError();
}
// Hs: the same H / hmax (the quotient in fp64) as three bf16 planes in
// gemmh_zrm_split_kernel's piece order (dfm_internal.h), a constant of the
// fit beside H32.  One workgroup per k-stage; thread (row a, k half kh) splits
// its 8 doubles (H's zero k-padding gives zero pieces; rows past T are zero).
__global__ __launch_bounds__(256) void fact_hsplit_kernel(const double *__restrict__ H, int64_t ldH, int T,
                                                          const double *__restrict__ hd, uint4 *__restrict__ Hs,
                                                          int mrows) {
  __shared__ double red[256];
  const int tid = threadIdx.x, ks = blockIdx.x;
  double mx = 0.0;
  for (int s = tid; s < T; s += 256) mx = fmax(mx, hd[s]);
  red[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmax(red[tid], red[tid + o]); __syncthreads(); }
  const double hmax = red[0] > 0.0 ? red[0] : 1.0;
  for (int e = tid; e < 2 * mrows; e += 256) {
    const int kh = e / mrows, a = e - kh * mrows;
    double x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = a < T ? H[(int64_t)a * ldH + 16 * ks + 8 * kh + j] / hmax : 0.0;
    uint4 ph, pm, pl;
    bf16_split3_piece(x, ph, pm, pl);
    uint4 *d = Hs + ((int64_t)ks * 6 + kh) * mrows + a;
    d[0] = ph; d[2 * (int64_t)mrows] = pm; d[4 * (int64_t)mrows] = pl;
  }
}
hipError_t launch_fact_hsplit(const double *H, int64_t ldH, int T, const double *hd, void *Hs, hipStream_t st) {
  if (ldH < (T + 15) / 16 * 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fact_hsplit_kernel, dim3((T + 15) / 16), dim3(256), 0, st, H, ldH, T, hd, (uint4 *)Hs, hsplit_rows(T));
  return hipGetLastError();
}
double fact_hmax(const double *hd_host, int T) {
  double mx = 0.0;
  for (int t = 0; t < T; ++t) mx = std::max(mx, hd_host[t]);   // (a NaN entry never wins, as fmax on the device)
  return mx > 0.0 ? mx : 1.0;
}

int fact_precompute(const double *Ep, int64_t ld, int T, int N, int r, const double *Lb, const double *Fb,
                    const double *H, int64_t ldH, double *EL, double *S, double *cF, double *hd, hipStream_t st) {
  hipLaunchKernelGGL(fact_pre_kernel, dim3((T + 3) / 4), dim3(256), 0, st, Ep, ld, T, N, r, Lb, Fb, H, ldH,
                     EL, S, cF, hd);
  hipLaunchKernelGGL(fact_cf_kernel, dim3((T + 255) / 256), dim3(256), 0, st, T, r, Fb, S, cF);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : 1000 + (int)e;
}

}  // namespace dfm
