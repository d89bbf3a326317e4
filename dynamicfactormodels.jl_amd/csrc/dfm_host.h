// dfm_host.h — private to the host layer of the C ABI of include/dfm.h
// (dfm_ctx.hip, dfm_panel.hip, dfm_fit.hip, dfm_boot.hip, dfm_windows.hip,
// dfm_mc.hip, dfm_em.hip): the context and model objects, error reporting,
// timing scopes, the owning device buffer and the small helpers those files
// share.  The criteria themselves are in dfm_criteria.h.  Host-side
// orchestration only; all arithmetic runs in the kernels of dfm_gram.hip (K1),
// dfm_eig.hip / dfm_fact.hip (K2), dfm_model.hip / dfm_chow.hip (K3).
#pragma once
#include "dfm_internal.h"
#include "../../include/dfm.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

using namespace dfm;

struct dfm_ctx {
  int device = 0;
  int refs = 1;            // the caller's handle + one per live dfm_model
  bool closed = false;
  hipStream_t own = nullptr, stream = nullptr;
  std::string err;
  double tol = 1e-12;   // residual <= tol * eigen-gap (see eig_gq_kernel)
  // bootstrap calls whose statistics depend on eigenvalues only: Ritz values
  // within this relative bound (Kato-Temple, check_converged); <= 0 = strict
  double tol_values = 1e-12;
  int maxit = 400, block = 0, poll = 4;
  bool timing = false;
  std::vector<hipEvent_t> pool;
  struct Pend { int cls; hipEvent_t a, b; };
  std::vector<Pend> pend;
  hipEvent_t cur_a[DFM_KC_COUNT] = {};
  double ms[DFM_KC_COUNT] = {};
  int64_t launches[DFM_KC_COUNT] = {};
  int64_t eig_batches = 0, eig_iters = 0, eig_iters_max = 0, rep_iters = 0, gemm_products = 0;
  int64_t gemm_products_f32 = 0;   // of the factored solver's replicate-products, those run in fp32 (host-counted)
  int64_t gemm_products_split_last = 0;   // the warm filter's last products run as six bf16 terms (0 or nb per solve)
  int64_t gemm_products_split3 = 0;       // of gemm_products_f32, those run as three bf16 terms ((d0 - 2) nb per solve)
  // factored runs accumulate {replicate-iterations, GEMM replicate-products}
  // here on the device (no host sync after the eigen loop); read on query
  long long *cnt_dev = nullptr;
  // expanding-windows scratch: one arena reused call to call (stream-ordered),
  // grown to the largest call's need — no per-call pool malloc/free on the host
  char *warena = nullptr;
  size_t warena_cap = 0, warena_need = 0;
  hipEvent_t gate = nullptr;   // bootstrap_lanes: the second lane starts behind the caller's prior work
  hipMemPool_t mpool = nullptr;  // this context's stream-ordered scratch (stream_malloc)
  PollBuf pollbuf;               // pinned convergence read-backs of the factored solver (host == nullptr: none)
  // the bootstrap lanes' contexts whose kernel timings this context reports:
  // merged when the timings are read (harvesting a lane's events after every
  // call put ~30 hipEventElapsedTime calls between a timed job's steps)
  std::vector<dfm_ctx *> kids;
};
inline const PollBuf *ctx_poll(const dfm_ctx *c) { return c->pollbuf.host ? &c->pollbuf : nullptr; }

// The host thread of a model's second bootstrap lane (bootstrap_lanes):
// persistent, so a call costs a hand-off, not a thread start.  Both sides of
// the hand-off spin briefly (kSpin) before blocking: in a run of jobs the next
// job, and the lane's finish, come within microseconds, and a condition
// variable wake-up (~10-20 us) sat in front of the lane's first kernel and
// behind its last one on every call.
struct LaneWorker {
  static constexpr std::chrono::microseconds kSpin{200};
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;   // guarded by mu
  std::atomic<bool> has{false}, done{false}, quit{false};
  std::thread th;   // last: starts after the members it uses
  LaneWorker() : th([this] { loop(); }) {}
  template <class F>
  static void spin(F ready) {
    const auto t0 = std::chrono::steady_clock::now();
    while (!ready() && std::chrono::steady_clock::now() - t0 < kSpin) __builtin_ia32_pause();
  }
  void loop() {
    for (;;) {
      spin([&] { return has.load(std::memory_order_acquire) || quit.load(std::memory_order_acquire); });
      std::function<void()> j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return has.load() || quit.load(); });
        if (quit.load()) return;
        j = std::move(job);
        has.store(false);
      }
      j();
      {
        std::lock_guard<std::mutex> g(mu);
        done.store(true, std::memory_order_release);
      }
      cv.notify_all();
    }
  }
  void run(std::function<void()> j) {
    {
      std::lock_guard<std::mutex> g(mu);
      job = std::move(j);
      done.store(false);
      has.store(true, std::memory_order_release);
    }
    cv.notify_all();
  }
  void wait() {
    spin([&] { return done.load(std::memory_order_acquire); });
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done.load(); });
  }
  ~LaneWorker() {
    {
      std::lock_guard<std::mutex> g(mu);
      quit.store(true);
    }
    cv.notify_all();
    th.join();
  }
};

struct dfm_model {
  dfm_ctx *ctx = nullptr;
  int T = 0, N = 0, q = 0, r = 0, crit = -1, kmax = 0, m = 0, orient = 0, k_eig = 0;
  bool swept = false;   // IC sweep ran (r chosen by criterion)
  int64_t ld = 0;
  double *Xp = nullptr, *Cp = nullptr, *Ep = nullptr, *y = nullptr, *w = nullptr;
  double *F = nullptr, *L = nullptr, *Ub = nullptr, *colssr = nullptr;
  std::vector<double> lam, coef, tstat, cov, resid, ic;
  double trace = 0, V = 0, critval = NAN, sigma2 = NAN;
  int64_t batch = 0;
  char *ws = nullptr;
  size_t ws_bytes = 0;
  // the sup-Chow sweep's workspace (dfm_chow_sweep.hip): bounded by the replicates per sweep launch, not by the
  // batch, and kept between calls (allocating and freeing it per job cost more than a sup-LM job's kernels)
  char *sw_ws = nullptr;
  size_t sw_bytes = 0;
  StatDesc *sd_dev = nullptr;
  int sd_cap = 0;
  std::vector<StatDesc> sd_host;   // what sd_dev holds (uploaded only when a call's descriptors differ)
  int *flag_dev = nullptr;
  // factored bootstrap (N > T): H = E E', EL = E L, S = L'L, cF, hd
  int mode = 0;   // 0 auto, 1 direct Gram, 2 factored
  bool fact_ready = false;
  int64_t ldH = 0;
  double *H = nullptr, *EL = nullptr, *S = nullptr, *cF = nullptr, *hd = nullptr;
  double *FtF = nullptr;   // F'F (16 x 16): the factored solver's middle Horner steps
  void *Hs = nullptr;      // the same as three bf16 planes (hsplit_bytes): those products as six bf16 terms
  float *H32 = nullptr;    // float(H / hmax) (T x ldH): the fp32 middle products of warm eigenvalue-rule solves
  double hmax = 0.0;       // max_t H[t][t]
  double *FSF = nullptr;   // F S F' (T x ldH): the direct path's identity-based replicate Grams
  // T >= N bootstrap Grams by one weighted-outer-product GEMM (gram_wk_*):
  // K = [E_s' E_s] lower-triangle pairs (Tp x ldk) and A0 = C'C (N x N)
  double *Kwk = nullptr, *A0wk = nullptr;
  // break blocks (src/DynamicFactorModel.jl:73, :98): first row, rows, Gram
  // size, per-block eigenvectors (Gram size x r) and loadings (N x r); block 0's
  // are aliased by Ub and L
  int nblk = 1;
  std::vector<int> ba, bt, bm;
  std::vector<double *> Ubs, Ls;   // Ls[j] = Lall + j N r (contiguous: the Chow kernels index blocks)
  double *Lall = nullptr;
  std::vector<std::vector<double>> blam;
  // dfm_chow: the all-variables statistics of the last break period asked for
  int64_t chow_bp = -1;
  std::vector<double> chow_cache;   // LR (N), LM (N), Wald (N)
  // the extra lanes of small factored bootstrap jobs (dfm_bootstrap_dev):
  // clones of this fit, each on its own context / stream of the same device
  // and driven by its own host thread, made on first use
  static constexpr int kMaxLanes = 4;
  dfm_model *lane[kMaxLanes - 1] = {};
  LaneWorker *lane_worker[kMaxLanes - 1] = {};
  bool is_lane = false;
  dfm_ctx *count_ctx = nullptr;   // a lane counts its GEMM products into its parent's context
  // a model of dfm_model_fit_em (dfm_em.hip): the completed panel in original units (column-major T x N) and
  // the moments of its last z-score; emX2 == nullptr for every other model
  double *emX2 = nullptr;
  std::vector<double> em_mu, em_sd;
};

namespace dfm {

// ---- dfm_ctx.hip
int fail(dfm_ctx *ctx, int code, const char *fmt, ...);
void timer_cb(void *p, int cls, int begin);
void merge_kid(dfm_ctx *ctx, dfm_ctx *kid);   // a lane context's timings into its parent's
void ctx_release(dfm_ctx *ctx);

#define HIPCHK(ctx, x)                                                                            \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess)                                                                         \
      return fail(ctx, 1000 + (int)e_, "HIP error %s at %s:%d", hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                      \
  } while (0)

struct Scope {
  dfm_ctx *c; int cls;
  Scope(dfm_ctx *c_, int k) : c(c_), cls(k) { timer_cb(c, cls, 1); }
  ~Scope() { timer_cb(c, cls, 0); }
};

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline bool chow_stat(int k) { return k >= DFM_STAT_LR && k <= DFM_STAT_WALD_ALL; }
// the sup-Chow stats over a range of break periods (dfm_chow_sweep.hip): arg0..arg1
inline bool sup_stat(int k) { return k >= DFM_STAT_SUPLR_ALL && k <= DFM_STAT_SUPWALD_ALL; }
inline bool all_var_stat(int k) { return (k >= DFM_STAT_LR_ALL && k <= DFM_STAT_WALD_ALL) || sup_stat(k); }
// values a stat adds to a replicate's row
inline int64_t stat_width(const dfm_model *m, int k) {
  if (all_var_stat(k)) return m->N;
  if (k == DFM_STAT_FACTORS) return (int64_t)m->T * m->r;
  if (k == DFM_STAT_LOADINGS) return (int64_t)m->N * m->r;
  return 1;
}
// T >= N, no breaks, small N: the batch's Grams by one weighted GEMM (gram_wk).
// Its prep kernel stages the replicate's draws and F (T x r) in LDS: only
// while that fits the default 64 KB dynamic-LDS launch; larger T r take the
// fused-gather K1 Gram (gram_kernel<COLS>).
inline bool use_gram_wk(const dfm_model *M) {
  return M->orient == 1 && M->nblk == 1 && M->N <= 256 && M->r >= 1 && M->r <= 16 &&
         gram_wk_prep_lds(M->T, M->r) <= 65536;
}

template <class T>
inline hipError_t dalloc(T **p, size_t n) {
  const hipError_t e = hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
  if (e == hipSuccess) DFM_POISON_SYNC(*p, std::max<size_t>(n, 1) * sizeof(T));
  return e;
}

// Owning device buffer (hipMalloc through dalloc / hipFree): move-only, freed on every return path
template <class T = double>
struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); return *this; }
  ~DevBuf() { hipFree(p); }
  hipError_t alloc(size_t n) {   // a block held from an earlier alloc is freed first
    if (p) hipFree(p);
    p = nullptr;
    return dalloc(&p, n);
  }
};

struct DevPanel {   // stream-ordered (pool) allocations: no device-wide sync in hipFree
  double *raw = nullptr, *P = nullptr;
  int64_t ld = 0;
  hipStream_t st = nullptr;
  ~DevPanel() {
    if (raw) hipFreeAsync(raw, st);
    if (P) hipFreeAsync(P, st);
  }
};
// ---- dfm_panel.hip: the model-less steps over one resident panel
int upload_panel(dfm_ctx *ctx, const double *X, int T, int N, int64_t ldx, DevPanel &dp, bool dev = false);
// Gram (m x m, m = orient == 0 ? T : N) of the T rows of src, under the Gram timing scope
hipError_t panel_gram(dfm_ctx *ctx, int orient, const PanelSrc &src, int T, int N, double *G);
// every eigenvalue of one m x m Gram, descending (m <= spectrum_any_max()); synchronises
int gram_spectrum(dfm_ctx *ctx, const double *G, int m, std::vector<double> &ev);
// the EigArgs fields a context decides: p, tol (a single fit's rule), maxit, poll, st, tf, tctx
EigArgs ctx_eig_args(dfm_ctx *ctx, int m, int k);
// Top-k eigenpairs + trace of one Gram.  ws == nullptr: run_eig allocates and frees the workspace and
// synchronises; a caller's ws (eig_workspace_bytes_padded, k inside the subspace block) adds neither.
// warm: m x k start vectors (nullptr: hashed start).
int run_eig(dfm_ctx *ctx, const double *G, int m, int k, double *lam, double *Uk, double *trace, int *status_dev,
            char *ws = nullptr, const double *warm = nullptr);
// row-major rows x cols device block -> column-major host array; synchronises
int read_rows_colmajor(dfm_ctx *ctx, const double *src, int rows, int cols, double *dst);

}  // namespace dfm
