// dfm_ctx.hip — the context of the C ABI (include/dfm.h): create / destroy /
// stream / solver parameters, the per-context memory pools behind
// stream_malloc, the device gate, kernel-class timing and the counters, the
// last-error text, and the host-side IC sweep.
#include "dfm_host.h"

static const char *kclass_names[DFM_KC_COUNT] = {"gram", "eig_gq", "eig_small", "eig_apply",
                                                 "eig_other", "factors", "ols", "stats", "chow",
                                                 "misc", "gemm"};

// stream -> the owning context's pool (stream_malloc); guarded: contexts are
// created, re-streamed and destroyed from any host thread.  One entry per
// context (a context re-registers after dfm_ctx_set_stream).  A stream that
// several contexts are bound to (dfm_ctx_set_stream with a shared external
// stream) is served by the device's default pool instead of either context's
// own: a context's pool then never holds blocks another context allocated,
// so destroying one context (hipMemPoolDestroy) cannot free memory still in
// flight on the other's calls.
static std::mutex g_pool_mu;
static std::vector<std::pair<hipStream_t, hipMemPool_t>> g_pools;
static void pool_register(hipStream_t st, hipMemPool_t pool) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  g_pools.emplace_back(st, pool);
}
static void pool_unregister(hipMemPool_t pool) {
  std::lock_guard<std::mutex> g(g_pool_mu);
  g_pools.erase(std::remove_if(g_pools.begin(), g_pools.end(), [&](const auto &e) { return e.second == pool; }),
                g_pools.end());
}
namespace dfm {
hipError_t stream_malloc(void **p, size_t bytes, hipStream_t st) {
  hipMemPool_t pool = nullptr;
  {
    std::lock_guard<std::mutex> g(g_pool_mu);
    int owners = 0;
    for (auto &e : g_pools)
      if (e.first == st) { pool = e.second; ++owners; }
    if (owners > 1) pool = nullptr;   // a shared stream: the default pool
  }
  const hipError_t e = pool ? hipMallocFromPoolAsync(p, bytes, pool, st) : hipMallocAsync(p, bytes, st);
  if (e == hipSuccess) DFM_POISON_ASYNC(*p, bytes, st);
  return e;
}

// The device gate (dfm_common.h): per device, a count of library calls in
// progress and a solo flag.  Shares wait only while a solo section runs
// (reader-preferring, so a call holding a share can always start more shared
// calls on other threads — dfm_bootstrap_multi's shards — without deadlocking
// behind a waiting solo); a solo section waits for the count to reach zero.
namespace {
struct DevGate {
  std::mutex mu;
  std::condition_variable cv;
  int shares = 0;
  bool solo = false;
};
constexpr int kGateDevs = 64;
DevGate g_gate[kGateDevs];
thread_local int t_shares[kGateDevs];   // this thread's nesting depth per device
}  // namespace
DeviceShare::DeviceShare(int device) : dev(device >= 0 && device < kGateDevs ? device : -1) {
  if (dev < 0 || t_shares[dev]++ > 0) return;
  DevGate &g = g_gate[dev];
  std::unique_lock<std::mutex> lk(g.mu);
  g.cv.wait(lk, [&] { return !g.solo; });
  ++g.shares;
}
DeviceShare::~DeviceShare() {
  if (dev < 0 || --t_shares[dev] > 0) return;
  DevGate &g = g_gate[dev];
  {
    std::lock_guard<std::mutex> lk(g.mu);
    --g.shares;
  }
  g.cv.notify_all();
}
DeviceSolo::DeviceSolo(int device) : dev(device >= 0 && device < kGateDevs ? device : -1) {
  if (dev < 0 || t_shares[dev] > 0) { dev = -1; return; }   // (nested in a shared call: would never drain)
  DevGate &g = g_gate[dev];
  std::unique_lock<std::mutex> lk(g.mu);
  g.cv.wait(lk, [&] { return !g.solo && g.shares == 0; });
  g.solo = true;
  held = true;
}
DeviceSolo::~DeviceSolo() {
  if (!held) return;
  DevGate &g = g_gate[dev];
  {
    std::lock_guard<std::mutex> lk(g.mu);
    g.solo = false;
  }
  g.cv.notify_all();
}

// ---- error text, kernel-class timing, teardown (dfm_host.h)
int fail(dfm_ctx *ctx, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

void timer_cb(void *p, int cls, int begin) {
  dfm_ctx *ctx = (dfm_ctx *)p;
  if (!ctx->timing) return;
  auto get = [&]() {
    hipEvent_t e;
    if (!ctx->pool.empty()) { e = ctx->pool.back(); ctx->pool.pop_back(); }
    else hipEventCreate(&e);
    return e;
  };
  if (begin) {
    ctx->cur_a[cls] = get();
    hipEventRecord(ctx->cur_a[cls], ctx->stream);
  } else {
    hipEvent_t b = get();
    hipEventRecord(b, ctx->stream);
    ctx->pend.push_back({cls, ctx->cur_a[cls], b});
    ctx->launches[cls]++;
  }
}
static void harvest(dfm_ctx *ctx) {
  if (ctx->pend.empty()) return;
  hipEventSynchronize(ctx->pend.back().b);
  for (auto &p : ctx->pend) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, p.a, p.b);
    ctx->ms[p.cls] += ms;
    ctx->pool.push_back(p.a);
    ctx->pool.push_back(p.b);
  }
  ctx->pend.clear();
}
// a lane context's timings into its parent's (read / reset time, lane teardown)
void merge_kid(dfm_ctx *ctx, dfm_ctx *kid) {
  harvest(kid);
  for (int i = 0; i < DFM_KC_COUNT; ++i) {
    ctx->ms[i] += kid->ms[i]; ctx->launches[i] += kid->launches[i];
    kid->ms[i] = 0; kid->launches[i] = 0;
  }
}
static void merge_kids(dfm_ctx *ctx) {
  for (dfm_ctx *k : ctx->kids) merge_kid(ctx, k);
}

void ctx_release(dfm_ctx *ctx) {
  if (--ctx->refs > 0) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  harvest(ctx);
  for (auto e : ctx->pool) hipEventDestroy(e);
  hipFree(ctx->cnt_dev);
  hipFree(ctx->warena);
  if (ctx->gate) hipEventDestroy(ctx->gate);
  if (ctx->pollbuf.host) {
    hipEventDestroy(ctx->pollbuf.ev[0]);
    hipEventDestroy(ctx->pollbuf.ev[1]);
    hipHostFree(ctx->pollbuf.host);
  }
  if (ctx->mpool) {
    pool_unregister(ctx->mpool);
    hipMemPoolDestroy(ctx->mpool);
  }
  if (ctx->own) hipStreamDestroy(ctx->own);
  delete ctx;
}

int ctx_fail(dfm_ctx *ctx, int code, const char *msg) { return fail(ctx, code, "%s", msg); }
hipStream_t ctx_stream(dfm_ctx *ctx) { return ctx->stream; }
int ctx_device(dfm_ctx *ctx) { return ctx->device; }
}  // namespace dfm

extern "C" {

int dfm_ctx_create(int device, dfm_ctx **out) {
  if (!out) return -1;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return -2;
  dfm_ctx *c = new dfm_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete c; return -3; }
  if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) { delete c; return -4; }
  c->stream = c->own;
  if (hipMalloc((void **)&c->cnt_dev, 2 * sizeof(long long)) != hipSuccess ||
      hipMemsetAsync(c->cnt_dev, 0, 2 * sizeof(long long), c->stream) != hipSuccess) {
    hipStreamDestroy(c->own);
    delete c;
    return -4;
  }
  {   // stream-ordered scratch (split-K Gram partials, eigen workspaces) from
      // the context's own pool, kept mapped between calls
    hipMemPoolProps props{};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = device;
    uint64_t keep = UINT64_MAX;
    if (hipMemPoolCreate(&c->mpool, &props) == hipSuccess) {
      hipMemPoolSetAttribute(c->mpool, hipMemPoolAttrReleaseThreshold, &keep);
      pool_register(c->stream, c->mpool);
    } else {
      c->mpool = nullptr;   // the default pool then serves this context (stream_malloc's fallback)
    }
    hipMemPool_t dp;
    if (hipDeviceGetDefaultMemPool(&dp, device) == hipSuccess) hipMemPoolSetAttribute(dp, hipMemPoolAttrReleaseThreshold, &keep);
  }
  {   // the factored solver's look-ahead polls (without them it polls blocking)
    PollBuf &pb = c->pollbuf;
    constexpr int kCap = 4096;
    if (hipHostMalloc((void **)&pb.host, kCap * sizeof(int), hipHostMallocDefault) == hipSuccess &&
        hipEventCreateWithFlags(&pb.ev[0], hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&pb.ev[1], hipEventDisableTiming) == hipSuccess) {
      pb.cap = kCap;
    } else {
      if (pb.ev[0]) hipEventDestroy(pb.ev[0]);
      if (pb.host) hipHostFree(pb.host);
      pb = PollBuf{};
    }
  }
  *out = c;
  return 0;
}

int dfm_ctx_destroy(dfm_ctx *ctx) {
  if (!ctx || ctx->closed) return -1;
  ctx->closed = true;
  ctx_release(ctx);
  return 0;
}

const char *dfm_last_error(const dfm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dfm_ctx_set_stream(dfm_ctx *ctx, void *s) {
  if (!ctx) return -1;
  if (ctx->mpool) pool_unregister(ctx->mpool);
  ctx->stream = s ? (hipStream_t)s : ctx->own;
  if (ctx->mpool) pool_register(ctx->stream, ctx->mpool);
  return 0;
}
int dfm_ctx_synchronize(dfm_ctx *ctx) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int dfm_ctx_set_eig_params(dfm_ctx *ctx, double tol, int max_iter, int block) {
  if (!ctx) return -1;
  if (tol > 0) ctx->tol = tol;
  if (max_iter > 0) ctx->maxit = max_iter;
  if (block >= 0) ctx->block = block;
  return 0;
}
int dfm_ctx_set_value_tol(dfm_ctx *ctx, double tol) {
  if (!ctx) return -1;
  ctx->tol_values = tol;
  return 0;
}
int dfm_ctx_enable_timing(dfm_ctx *ctx, int enable) {
  if (!ctx) return -1;
  ctx->timing = enable != 0;
  if (ctx->timing) {   // events made up front, not one hipEventCreate per timed launch inside the jobs
    hipSetDevice(ctx->device);
    auto fill = [](dfm_ctx *c) {
      while (c->pool.size() < 1024) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) break;
        c->pool.push_back(e);
      }
    };
    fill(ctx);
    for (dfm_ctx *c : ctx->kids) fill(c);
  }
  return 0;
}
int dfm_ctx_read_timing(dfm_ctx *ctx, double *ms_out, int64_t *launches_out, int cap) {
  if (!ctx) return -1;
  harvest(ctx);
  merge_kids(ctx);
  const int n = std::min(cap, (int)DFM_KC_COUNT);
  for (int i = 0; i < n; ++i) {
    if (ms_out) ms_out[i] = ctx->ms[i];
    if (launches_out) launches_out[i] = ctx->launches[i];
  }
  return n;
}
int dfm_ctx_reset_timing(dfm_ctx *ctx) {
  if (!ctx) return -1;
  harvest(ctx);
  merge_kids(ctx);
  for (int i = 0; i < DFM_KC_COUNT; ++i) { ctx->ms[i] = 0; ctx->launches[i] = 0; }
  ctx->eig_batches = ctx->eig_iters = ctx->eig_iters_max = ctx->rep_iters = ctx->gemm_products = 0;
  ctx->gemm_products_f32 = ctx->gemm_products_split_last = ctx->gemm_products_split3 = 0;
  hipMemsetAsync(ctx->cnt_dev, 0, 2 * sizeof(long long), ctx->stream);
  return 0;
}
// host totals + the device-side counters of factored runs (one sync, on query)
static void read_counts(dfm_ctx *ctx, int64_t *rep_iters, int64_t *products) {
  long long c[2] = {0, 0};
  hipMemcpyAsync(c, ctx->cnt_dev, sizeof(c), hipMemcpyDeviceToHost, ctx->stream);
  hipStreamSynchronize(ctx->stream);
  if (rep_iters) *rep_iters = ctx->rep_iters + c[0];
  if (products) *products = ctx->gemm_products + c[1];
}
int dfm_ctx_eig_stats(dfm_ctx *ctx, int64_t *batches, int64_t *iters_total, int64_t *iters_max) {
  if (!ctx) return -1;
  if (batches) *batches = ctx->eig_batches;
  if (iters_total) *iters_total = ctx->eig_iters;
  if (iters_max) *iters_max = ctx->eig_iters_max;
  return 0;
}
int dfm_ctx_gemm_products(dfm_ctx *ctx, int64_t *products) {
  if (!ctx || !products) return -1;
  read_counts(ctx, nullptr, products);
  return 0;
}
int dfm_ctx_gemm_products_f32(dfm_ctx *ctx, int64_t *products) {
  if (!ctx || !products) return -1;
  *products = ctx->gemm_products_f32;
  return 0;
}
int dfm_ctx_gemm_products_split3(dfm_ctx *ctx, int64_t *products) {
  if (!ctx || !products) return -1;
  *products = ctx->gemm_products_split3;
  return 0;
}
int dfm_ctx_gemm_products_split_last(dfm_ctx *ctx, int64_t *products) {
  if (!ctx || !products) return -1;
  *products = ctx->gemm_products_split_last;
  return 0;
}
int dfm_ctx_rep_iters(dfm_ctx *ctx, int64_t *rep_iters) {
  if (!ctx || !rep_iters) return -1;
  read_counts(ctx, rep_iters, nullptr);
  return 0;
}
const char *dfm_kernel_class_name(int cls) {
  return (cls >= 0 && cls < DFM_KC_COUNT) ? kclass_names[cls] : "?";
}
int dfm_full_spectrum_max(void) { return spectrum_any_max(); }

int dfm_ic_sweep(const double *eig, int n_eig, int kmax, double trace, int64_t T, int64_t N,
                 double sigma2, double *out) {
  if (!eig || !out || kmax < 1 || n_eig < kmax || T < 1 || N < 1) return -1;
  if (sigma2 < 0) {   // the trace minus the top ceil(m/2) eigenvalues
    const int m = (int)std::min(T, N);
    if (n_eig < ceil_half(m)) return -2;
    sigma2 = sigma2_minus_top(trace, eig, m, (double)N * (double)T);
  }
  criteria_sweep(eig, kmax, trace, sigma2, T, N, out);
  return 0;
}

}  // extern "C"
