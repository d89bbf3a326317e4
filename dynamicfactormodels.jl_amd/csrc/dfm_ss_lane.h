// dfm_ss_lane.h — what the simulation smoother (dfm_ss_sim.hip) and the news
// decomposition (dfm_ss_news.hip) share on the device: the record of a row
// that ss_gain_kernel (dfm_ss_lane.hip) writes, and the core of the
// one-lane-per-column kernels that read it (ss_sim_kernel, ss_news_kernel).
#pragma once
#include "dfm_common.h"
#include "dfm_ss_host.h"

namespace dfm {

// ------------------------------------------------------------- a row's record
// Per class c < ncls: the flag n^c_t > 0 (1.0 / 0.0), [b_t (r)], C_t (r x r),
// [R_t (r x r, lower)], K_t (s x r) — what a forward pass reads — then J_t
// (s x s), all row-major.  sim: with the simulation smoother's b_t and R_t.
__host__ __device__ constexpr int ss_rec_C(int r, bool sim) { return 1 + (sim ? r : 0); }
__host__ __device__ constexpr int ss_rec_K(int r, bool sim) { return ss_rec_C(r, sim) + (sim ? 2 : 1) * r * r; }
__host__ __device__ constexpr int ss_rec_cls(int r, int s, bool sim) { return ss_rec_K(r, sim) + s * r; }
__host__ __device__ constexpr int ss_rec_fwd(int r, int s, int ncls, bool sim) { return ncls * ss_rec_cls(r, s, sim); }
__host__ __device__ constexpr int ss_rec_len(int r, int s, int ncls, bool sim) { return ss_rec_fwd(r, s, ncls, sim) + s * s; }

// What a lane kernel stages of a record at a time: the forward part or J_t.
__host__ __device__ constexpr int ss_rec_stage(int r, int s, int ncls, bool sim) {
  return ss_rec_fwd(r, s, ncls, sim) > s * s ? ss_rec_fwd(r, s, ncls, sim) : s * s;
}
// The registers per lane that hold the wave's next staged part: 64 of them cover it at the limits.
constexpr int ss_lane_pre(int ncls, bool sim) { return (ss_rec_stage(SS_RMAX, SS_SMAX, ncls, sim) + 63) / 64; }
// A lane's own next row: 2 r normals or s entries of c_t|t (SS_LANE_IN), r entries of an output row (SS_LANE_OUT).
constexpr int SS_LANE_IN = SS_SMAX, SS_LANE_OUT = SS_RMAX;
static_assert(SS_LANE_IN >= 2 * SS_RMAX && SS_LANE_IN >= SS_SMAX, "a lane's next row does not fit its registers");

// LDS doubles of a lane kernel: its constants, one staged part of a record and
// cols columns of 64 lanes.
inline size_t ss_lane_lds(int cst, int r, int s, int ncls, bool sim, int cols) {
  return (size_t)cst + ss_rec_stage(r, s, ncls, sim) + (size_t)cols * 64;
}

// v + sum_{k<n} a[k] x[64 k] (NEG: v - sum), the products added in the order of k: a from the
// staged record or the constants (a broadcast read), x a lane's column.  Eight
// pairs are read before their multiply-adds run, so a round costs one LDS
// latency, not eight: the chain of a lane is serial and nothing else hides it.
template <bool NEG>
DFM_DEV double sim_dot(double v, const double *a, const double *x, int n) {
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double av[8], xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      av[q] = a[k + q];
      xv[q] = x[(k + q) * 64];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v = fma(NEG ? -av[q] : av[q], xv[q], v);
  }
  for (; k < n; ++k) v = fma(NEG ? -a[k] : a[k], x[k * 64], v);
  return v;
}

// ------------------------------------------------------------- the lane core
// One wave per workgroup, one lane per column (a draw, a release).  Element k
// of a lane's vector is at [k * 64 + lane] of its LDS region: a wave's access
// is one conflict-free row, and every read of the staged record is a
// broadcast.  What the next row reads from global memory — its record, and the
// lane's own entries — is fetched into registers while this row is computed,
// so a row waits for no load of its own; the two barriers of stage() fence the
// staging buffer.  No call sits inside a lane's condition.
// NCLS, SIM: the record the kernel reads.
template <int NCLS, bool SIM>
struct SsLane {
  static constexpr int PRE = ss_lane_pre(NCLS, SIM);
  static_assert(64 * PRE >= ss_rec_fwd(SS_RMAX, SS_SMAX, NCLS, SIM) && 64 * PRE >= SS_SMAX * SS_SMAX,
                "the staging registers do not cover the forward record and J_t");
  const int lane, r, s;
  const double *const Tmr;   // LDS: the companion matrix's first r rows (r x s)
  double *const st;          // LDS: the staged part of a record
  double *const W;           // LDS: this lane's work column, s entries at the least
  double pre[PRE], lp[SS_LANE_IN];

  DFM_DEV SsLane(int lane_, int r_, int s_, const double *Tmr_, double *st_, double *W_)
      : lane(lane_), r(r_), s(s_), Tmr(Tmr_), st(st_), W(W_) {}

  // the wave's next staged part, len doubles at src, into registers
  DFM_DEV void fetch(const double *src, int len) {
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = lane + 64 * q;
      pre[q] = e < len ? src[e] : 0.0;
    }
  }
  // ... and from there into the staging buffer
  DFM_DEV void stage(int len) {
    __syncthreads();   // the previous part is read
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = lane + 64 * q;
      if (e < len) st[e] = pre[q];
    }
    __syncthreads();
  }
  // the lane's own next row, cnt entries step apart at base (zeros without have), into registers
  DFM_DEV void lfetch(bool have, const double *base, int64_t step, int cnt) {
#pragma unroll
    for (int q = 0; q < SS_LANE_IN; ++q) lp[q] = (have && q < cnt) ? base[q * step] : 0.0;
  }
  // ... and from there into the column x
  DFM_DEV void lput(double *x, int cnt) {
#pragma unroll
    for (int q = 0; q < SS_LANE_IN; ++q)
      if (q < cnt) x[q * 64] = lp[q];
  }
  // x <- Tm x on a lane's column: the first r rows by dot products into W, the rest a shift
  DFM_DEV void advance(double *x) {
    for (int i = 0; i < r; ++i) W[i * 64] = sim_dot<false>(0.0, Tmr + i * s, x, s);
    for (int i = s - 1; i >= r; --i) x[i * 64] = x[(i - r) * 64];
    for (int i = 0; i < r; ++i) x[i * 64] = W[i * 64];
  }
  // One backward step with J_t staged: c holds c_{t+1|T} and receives c_t|T =
  // c_t|t + J_t (c_{t+1|T} - Tm c_t|t), cf holds c_t|t.
  DFM_DEV void back(double *c, const double *cf) {
    for (int i = 0; i < s; ++i) {
      const double v = i < r ? sim_dot<false>(0.0, Tmr + i * s, cf, s) : cf[(i - r) * 64];
      W[i * 64] = c[i * 64] - v;
    }
    for (int i = 0; i < s; ++i) c[i * 64] = sim_dot<false>(cf[i * 64], st + i * s, W, s);
  }
};

}  // namespace dfm
