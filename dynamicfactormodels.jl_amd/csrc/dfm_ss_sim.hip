// dfm_ss_sim.hip — the simulation smoother of Durbin & Koopman (2002) on top of
// the state-space pass: D joint draws of the factor path given the observed
// entries of one panel (dfm_ss_simulate; the algorithm, the layout of the
// normals and the return codes are stated in include/dfm.h).
//
// The smoother's own launches run once on the panel (ss_smooth_core of
// dfm_ss.hip, which hands over what they leave on the device and the geometry
// they ran at), then the driver of dfm_ss_lane.hip runs ss_gain_kernel (K_t,
// J_t, and for this file b_t and R_t, one record per row) and, per pass,
//   ss_sim_kernel           one lane per draw on the lane core of
//                           dfm_ss_lane.h: alpha+, b* and c forwards, c_t|T
//                           backwards
// and brings the pass's draws to the caller's [draw][t][k].
// The covariance recursion is never repeated: a draw is a mean-only recursion
// of about 3 r s multiply-adds per row.  No lane reads another lane's values,
// so a draw depends on neither D, its position nor its pass, and a NaN among
// its normals stays in it.
#include "dfm_host.h"
#include "dfm_ss_host.h"
#include "dfm_ss_lane.h"

namespace {

struct SsSimArgs {
  int Tt, r, s, n;       // n: the pass's draws
  int64_t ldz;
  const double *z;       // the pass's first draw: draw d's entry e at z[e ldz + d]
  const double *rec;     // ss_gain_kernel's records (one class, with b_t and R_t)
  const double *cst;     // a0 (s), L0 (s x s), the companion matrix's first r rows (r x s), Lq (r x r), row-major
  double *cf, *out;      // c_t|t [Tt][s][n] and the draws [Tt][r][n]
};

// Draw blockIdx.x * 64 + lane of the pass.  LDS: the companion rows, Lq, the
// staged record, and the columns of alpha+ (s), c (s) and the work vector
// (max(s, 2 r)).  A lane past the pass's last draw reads zeros for its normals
// and stores nothing.
__global__ __launch_bounds__(64) void ss_sim_kernel(SsSimArgs g) {
  extern __shared__ __attribute__((aligned(16))) double sim_lds[];
  const int Tt = g.Tt, r = g.r, s = g.s, n = g.n, lane = threadIdx.x;
  const int nf = ss_rec_fwd(r, s, 1, true), nrec = nf + s * s, ss = s * s;
  double *Tmr = sim_lds, *Lq = Tmr + r * s, *st = Lq + r * r;
  double *A = st + ss_rec_stage(r, s, 1, true) + lane, *Cc = A + s * 64, *W = Cc + s * 64;   // this lane's columns
  const int64_t d = (int64_t)blockIdx.x * 64 + lane;
  const bool act = d < n;
  const double *zc = g.z + (act ? d : 0);
  auto zat = [&](int64_t e) { return act ? zc[e * g.ldz] : 0.0; };
  const double *a0 = g.cst, *L0 = a0 + s;
  for (int e = lane; e < r * s + r * r; e += 64) Tmr[e] = g.cst[s + ss + e];   // Tmr and Lq are adjacent on both sides
  SsLane<1, true> ln(lane, r, s, Tmr, st, W);
  double lo[SS_LANE_OUT];   // the lane's own next output row
  for (int i = 0; i < s; ++i) Cc[i * 64] = 0.0;
  ln.fetch(g.rec, nf);
  ln.lfetch(act, zc + s * g.ldz, g.ldz, 2 * r);
  // ---------------------------------------------------------------- forwards
  for (int t = 0; t < Tt; ++t) {
    ln.stage(nf);
    if (t == 0) {   // alpha+_0 = a0 + L0 z0
      for (int k = 0; k < s; ++k) W[k * 64] = zat(k);
      for (int i = 0; i < s; ++i) A[i * 64] = sim_dot<false>(a0[i], L0 + i * s, W, i + 1);
    } else {
      ln.advance(A);
    }
    ln.lput(W, 2 * r);   // u_t at W[0, r), zeta_t at W[r, 2 r)
    if (t + 1 < Tt) {
      ln.fetch(g.rec + (int64_t)(t + 1) * nrec, nf);
      ln.lfetch(act, zc + (s + 2 * (int64_t)r * (t + 1)) * g.ldz, g.ldz, 2 * r);
    } else if (Tt >= 2) {
      ln.fetch(g.rec + (int64_t)(Tt - 2) * nrec + nf, ss);
    }
    if (t > 0)      // alpha+_t = Tm alpha+_{t-1} + [Lq u_t; 0]
      for (int i = 0; i < r; ++i) A[i * 64] = sim_dot<false>(A[i * 64], Lq + i * r, W, i + 1);
    if (act)
      for (int i = 0; i < r; ++i) g.out[((int64_t)t * r + i) * n + d] = A[i * 64];
    if (st[0] != 0.0) {
      const double *b = st + 1, *C = st + ss_rec_C(r, true), *R = C + r * r, *K = st + ss_rec_K(r, true);
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
    ln.advance(Cc);
  }
  // --------------------------------------------------------------- backwards
  if (act)
    for (int i = 0; i < r; ++i) g.out[((int64_t)(Tt - 1) * r + i) * n + d] += Cc[i * 64];
  const double *cfd = g.cf + (act ? d : 0);
  double *outd = g.out + (act ? d : 0);
  if (Tt >= 2) ln.lfetch(act, cfd + (int64_t)(Tt - 2) * s * n, n, s);
  for (int t = Tt - 2; t >= 0; --t) {
    ln.stage(ss);   // J_t
    ln.lput(A, s);  // c_t|t
#pragma unroll
    for (int q = 0; q < SS_LANE_OUT; ++q) lo[q] = (act && q < r) ? outd[((int64_t)t * r + q) * n] : 0.0;   // f+_t
    if (t >= 1) {
      ln.fetch(g.rec + (int64_t)(t - 1) * nrec + nf, ss);
      ln.lfetch(act, cfd + (int64_t)(t - 1) * s * n, n, s);
    }
    ln.back(Cc, A);
#pragma unroll
    for (int q = 0; q < SS_LANE_OUT; ++q)
      if (act && q < r) outd[((int64_t)t * r + q) * n] = lo[q] + Cc[q * 64];
  }
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
    const int Tt = k.g.Tt, r = k.g.r, s = k.g.s, ss = s * s;
    const int64_t nz = ss_sim_nz(Tt, r, s);
    SsSimArgs sa{};
    SsLaneJob job{};
    job.sim = true;
    job.cst.resize((size_t)s + ss + r * s + r * r);   // a0, L0, the companion matrix's first r rows, Lq
    std::copy(k.ha0, k.ha0 + s, job.cst.begin());
    ss_psd_cholesky(k.hP0, s, &job.cst[s]);
    std::copy(k.hTm, k.hTm + r * s, &job.cst[(size_t)s + ss]);
    std::copy(Lq.begin(), Lq.end(), &job.cst[(size_t)s + ss + r * s]);
    job.kernel = (const void *)ss_sim_kernel;
    job.args = &sa;
    job.lds = ss_lane_lds(r * s + r * r, r, s, 1, true, 2 * s + std::max(s, 2 * r)) * 8;
    job.count = D;
    job.per_pass = ss_sim_draws_per_pass(Tt, r, s, D, pass_draws, !z_dev);
    job.per_out = (size_t)Tt * r;
    job.planes = 1;
    job.host[0] = draws;
    StreamBuf dz;
    if (!z_dev) HIPCHK(ctx, dz.alloc((size_t)job.per_pass * nz * 8, ctx->stream));
    return ss_lane_run(ctx, k, job, [&](int64_t d0, int64_t n, const SsLaneBufs &b) {
      const double *zp = z + d0;
      int64_t ld = ldz;
      if (!z_dev) {
        HIPCHK(ctx, hipMemcpy2DAsync(dz.p, (size_t)n * 8, zp, (size_t)ldz * 8, (size_t)n * 8, (size_t)nz,
                                     hipMemcpyHostToDevice, b.st));
        zp = (const double *)dz.p;
        ld = n;
      }
      sa = SsSimArgs{Tt, r, s, (int)n, ld, zp, b.rec, b.cst, b.cf, b.out};
      return 0;
    });
  }
};

}  // namespace

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
