// dfm_ss_news.hip — the news decomposition of Banbura & Modugno (2014) on top
// of the state-space pass: which release moved the smoothed path between two
// vintages of one panel, and by how much (dfm_ss_news; the mathematics, the
// layouts and the return codes are stated in include/dfm.h).
//
// The smoother's own launches run on X_old, X_rev and X_new (ss_smooth_core of
// dfm_ss.hip); the last run hands over what it leaves on the device, then the
// driver of dfm_ss_lane.hip runs ss_gain_kernel (per class C^c_t and K^c_t,
// then J_t, one record per row) and, per pass,
//   ss_news_kernel        one lane per release on the lane core of
//                         dfm_ss_lane.h: the impulse response c forwards from
//                         the lane's own row t_j, c_t|T backwards down to t_lo
// and brings the pass's weights to the caller's [release][t][k].
// No lane reads another lane's values: a release's weights depend on neither
// J, its lane nor its pass.
#include "dfm_host.h"
#include "dfm_ss_host.h"
#include "dfm_ss_lane.h"

namespace {

struct NewsArgs {
  int Tt, t_lo, r, s, n, nw;   // n: the pass's releases
  const int *row;              // the pass's releases: t_j (n), then the class c(i_j) (n)
  const double *beta;          // lambda_{i_j} / sigma^2_{i_j}: entry k of release d at beta[k n + d]
  const double *rec;           // ss_gain_kernel's records (a class per frequency, without b_t and R_t)
  const double *cst;           // the companion matrix's first r rows (r x s row-major), then the weights (SS_WMAX)
  double *cf;                  // c_t|t [Tt][s][n]
  double *wf, *wa;             // c_t|T[:r] and Z_l c_t|T, [Tt - t_lo][r][n] each (wa: MF only)
};

// Release blockIdx.x * 64 + lane of the pass.  LDS: the companion rows, the
// weights, the staged record, and the columns of c (s), c_t|t (s), the work
// vector (max(s, 2 r)) and beta (r).  The releases are sorted by row, so the
// wave's forward loop starts at its first lane's t_j; a lane does nothing
// before its own row (its c is zero there).  A lane past the pass's last
// release never starts and stores nothing.
template <bool MF>
__global__ __launch_bounds__(64) void ss_news_kernel(NewsArgs g) {
  extern __shared__ __attribute__((aligned(16))) double news_lds[];
  constexpr int NCLS = MF ? 2 : 1;
  const int Tt = g.Tt, t_lo = g.t_lo, r = g.r, s = g.s, n = g.n, nw = g.nw, lane = threadIdx.x;
  const int ncl = ss_rec_cls(r, s, false), nf = NCLS * ncl, nrec = nf + s * s, ss = s * s;
  double *Tmr = news_lds, *wl = Tmr + r * s, *st = wl + SS_WMAX;
  double *Cc = st + ss_rec_stage(r, s, NCLS, false) + lane, *A = Cc + s * 64, *W = A + s * 64;   // this lane's columns
  double *B = W + (s > 2 * r ? s : 2 * r) * 64;
  const int64_t d = (int64_t)blockIdx.x * 64 + lane;
  const bool act = d < n;
  const int tj = act ? g.row[d] : Tt, cj = act ? g.row[n + d] : 0;
  const int t0 = g.row[(int64_t)blockIdx.x * 64];   // the wave's smallest row
  for (int e = lane; e < r * s + SS_WMAX; e += 64) Tmr[e] = g.cst[e];   // Tmr and wl are adjacent on both sides
  SsLane<NCLS, false> ln(lane, r, s, Tmr, st, W);
  // the lane's own c_t|t; that of a row before the wave's first is zero and was not stored
  auto lfetch = [&](int t) { ln.lfetch(act && t >= t0, g.cf + (int64_t)t * s * n + d, n, s); };
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
  ln.fetch(g.rec + (int64_t)t0 * nrec, nf);
  // ---------------------------------------------------------------- forwards
  for (int t = t0; t < Tt; ++t) {
    ln.stage(nf);
    if (t + 1 < Tt) ln.fetch(g.rec + (int64_t)(t + 1) * nrec, nf);
    else if (Tt >= 2) ln.fetch(g.rec + (int64_t)(Tt - 2) * nrec + nf, ss);
    const bool on = t >= tj;
    if (on) {
#pragma unroll
      for (int c = 0; c < NCLS; ++c) {
        const double *rc = st + c * ncl;
        if (rc[0] == 0.0) continue;
        const double *C = rc + ss_rec_C(r, false), *K = rc + ss_rec_K(r, false);
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
    if (on) ln.advance(Cc);
  }
  // --------------------------------------------------------------- backwards
  emit(Tt - 1);
  if (Tt - 2 >= t_lo) lfetch(Tt - 2);
  for (int t = Tt - 2; t >= t_lo; --t) {
    ln.stage(ss);    // J_t
    ln.lput(A, s);   // c_t|t
    if (t - 1 >= t_lo) {
      ln.fetch(g.rec + (int64_t)(t - 1) * nrec + nf, ss);
      lfetch(t - 1);
    }
    ln.back(Cc, A);
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
    const int Tt = G.Tt, r = G.r, s = G.s, ncls = G.mixed ? 2 : 1;
    NewsArgs na{};
    SsLaneJob job{};
    job.nw = nw;
    job.w_at = r * s;
    job.cst.assign((size_t)r * s + SS_WMAX, 0.0);   // the companion matrix's first r rows, the weights
    std::copy(k.hTm, k.hTm + r * s, job.cst.begin());
    if (G.mixed) std::copy(w, w + nw, &job.cst[(size_t)r * s]);
    job.kernel = G.mixed ? (const void *)ss_news_kernel<true> : (const void *)ss_news_kernel<false>;
    job.args = &na;
    job.lds = ss_lane_lds(r * s + SS_WMAX, r, s, ncls, false, 2 * s + std::max(s, 2 * r) + r) * 8;
    job.count = J;
    job.per_pass = ss_news_releases_per_pass(Tt, t_lo, r, s, G.mixed, J, pass_releases);
    job.per_out = (size_t)(Tt - t_lo) * r;
    job.planes = ncls;
    job.host[0] = wf;
    job.host[1] = G.mixed ? wa : nullptr;
    const int64_t np = job.per_pass;
    StreamBuf drow, dbeta;
    HIPCHK(ctx, drow.alloc((size_t)np * 2 * 4, ctx->stream));
    HIPCHK(ctx, dbeta.alloc((size_t)np * r * 8, ctx->stream));
    std::vector<double> hb((size_t)np * r);   // both reused after the pass's stream synchronise
    std::vector<int> hrow((size_t)np * 2);
    return ss_lane_run(ctx, k, job, [&](int64_t j0, int64_t n, const SsLaneBufs &b) {
      for (int64_t d = 0; d < n; ++d) {
        const int64_t i = rel_i[j0 + d];
        hrow[d] = (int)rel_t[j0 + d];
        hrow[n + d] = G.mixed && low[i] ? 1 : 0;
        for (int q = 0; q < r; ++q) hb[(size_t)q * n + d] = L[(size_t)q * G.N + i] / sigma2[i];
      }
      HIPCHK(ctx, hipMemcpyAsync(drow.p, hrow.data(), (size_t)n * 2 * 4, hipMemcpyHostToDevice, b.st));
      HIPCHK(ctx, hipMemcpyAsync(dbeta.p, hb.data(), (size_t)n * r * 8, hipMemcpyHostToDevice, b.st));
      na = NewsArgs{Tt, t_lo, r, s, (int)n, nw, (const int *)drow.p, (const double *)dbeta.p, b.rec, b.cst, b.cf, b.out,
                    b.out + (size_t)n * job.per_out};
      return 0;
    });
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
