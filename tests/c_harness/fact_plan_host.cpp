// Stand-alone check of csrc/dfm_fact_plan.h with a plain C++ compiler: no HIP,
// nothing linked from the project.  The reference is the rule as
// eig_run_fact2_t spelled it before the header existed — its chain of
// booleans, the two ternaries of its step-0 loop, the Z0 format expression,
// the two counter lines and the pad-row condition, copied — and every field of
// plan_first_filter's plan is held against it over a sweep of the solver's
// inputs and all settings of the on/off switches.  Every plan of the sweep
// must be consistent(), and three hand-broken ones must not be.
#include "dfm_fact_plan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

using namespace dfm;

static long failures = 0, plans = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (failures < 20) std::printf("FAILED line %d (%s): %s\n", __LINE__, what, #cond); \
      ++failures;                                                                \
    }                                                                            \
  } while (0)

// ---- the rule as it stood (first_filter_degree with the default cap, then eig_run_fact2_t's lines)
static int ref_first_filter_degree(double spread) {
  const double ratio = std::max(1.0001, 1.1 * spread);
  const int d = (int)std::floor(std::log(1e6) / std::log(ratio));
  return std::max(2, std::min(6, d));
}
struct Ref {
  bool warm_started, mid, skip0, stg_ok, lowp, split, split_last, nopf;
  int d0, z32;
};
static Ref ref_rule(const FilterPlanIn &in, const FactSwitches &sw) {
  const int m = in.T, k = in.k, p = in.p, maxit = in.maxit, P = in.P, pz = (p + 1) & ~1;
  const bool H32 = in.has_H32, Hs = in.has_Hs;
  const bool warm_keep_step0 = sw.keep_step0, fact_f32_off = sw.f32_off, fact_split_off = sw.split_off,
             fact_split_last_off = sw.split_last_off, fact_pf_stored = sw.pf_stored;
  Ref r;
  const bool warm_started = in.warm && in.kw >= k && in.spread >= 1.0;
  const int d0 = warm_started ? ref_first_filter_degree(in.spread) : 2;
  const bool mid = d0 >= 3;
  const double bfix = 0.21 * in.lamk;
  const bool skip0 = warm_started && mid && maxit >= 2 && bfix > 0.0 && p <= 32 && !warm_keep_step0;
  const bool stg_ok = P == 16 && in.r <= 8 && (in.r & 1) == 0 && pz <= 16;
  const bool lowp = skip0 && in.tol < 0.0 && H32 && std::isfinite(in.hmax) && in.hmax > 0.0 && m >= 16 && !fact_f32_off;
  const bool split = lowp && Hs && !fact_split_off;
  const bool split_last = split && !fact_split_last_off;
  const bool nopf = skip0 && in.fscale > 0.0 && in.kw >= in.r && !fact_pf_stored;
  r.warm_started = warm_started; r.d0 = d0; r.mid = mid; r.skip0 = skip0; r.stg_ok = stg_ok; r.lowp = lowp;
  r.split = split; r.split_last = split_last; r.nopf = nopf;
  r.z32 = split ? 2 : lowp ? 1 : 0;
  return r;
}
// the step-0 loop's product: (lowp && sp < d0) ? hz32() : (split_last && sp == d0) ? hz_split_rows() : hz(false),
// hz32 launching the split kernel if split, else the fp32 one
static HzProduct ref_product(const Ref &r, int sp) {
  const bool lowp = r.lowp, split = r.split, split_last = r.split_last;
  const int d0 = r.d0;
  return (lowp && sp < d0) ? (split ? HzProduct::Split : HzProduct::F32)
                           : (split_last && sp == d0) ? HzProduct::SplitRows : HzProduct::F64;
}
// ... and its middle step's LP
static int ref_lp(const Ref &r, int sp) {
  const bool lowp = r.lowp, split = r.split, split_last = r.split_last;
  const int d0 = r.d0;
  return !lowp ? 0 : (sp < d0 - 1 || split_last) ? (split ? 3 : 1) : 2;
}

static void check_plan(const FilterPlanIn &in, const FactSwitches &sw, const char *what) {
  const Ref r = ref_rule(in, sw);
  const FilterPlan pl = plan_first_filter(in, sw);
  ++plans;
  CHECK(pl.warm_started == r.warm_started && pl.d0 == r.d0 && pl.mid == r.mid && pl.skip0 == r.skip0);
  CHECK(pl.stg_ok == r.stg_ok && pl.nopf == r.nopf);
  CHECK((int)pl.z0 == r.z32);   // 0 = fp64, 1 = float, 2 = bf16 planes
  CHECK(pl.d0 >= 2 && pl.d0 <= kFilterDMax);
  static const HzFmt lp_in[4] = {HzFmt::Rows64, HzFmt::Chunk32, HzFmt::Chunk32, HzFmt::Chunk32};
  static const ZFmt lp_out[4] = {ZFmt::F64, ZFmt::F32, ZFmt::F64, ZFmt::Split};
  for (int sp = 1; sp <= pl.d0; ++sp) {
    CHECK(pl.product[sp] == ref_product(r, sp));
    if (sp < pl.d0) {
      const int lp = ref_lp(r, sp);
      CHECK(pl.mid_in[sp] == lp_in[lp] && pl.mid_out[sp] == lp_out[lp]);
    }
  }
  // hz_split_rows ran for product d0 iff split_last, and zeroed the pad rows iff (m & 15)
  CHECK(pl.zero_zpad == (r.split_last && (in.T & 15) != 0));
  for (int64_t nb : {1, 64, 1250}) {
    CHECK((int64_t)pl.products_f32 * nb == (r.lowp ? (int64_t)(r.d0 - 1) * nb : 0));
    CHECK((int64_t)pl.products_split_last * nb == (r.split_last ? (int64_t)nb : 0));
  }
  if (!pl.consistent() && failures < 5)
    std::printf("T=%d r=%d p=%d tol=%g H32=%d Hs=%d hmax=%g spread=%g maxit=%d kw=%d lamk=%g d0=%d skip0=%d z0=%d zpad=%d\n",
                in.T, in.r, in.p, in.tol, in.has_H32, in.has_Hs, in.hmax, in.spread, in.maxit, in.kw, in.lamk, pl.d0,
                pl.skip0, (int)pl.z0, pl.zero_zpad);
  CHECK(pl.consistent());
}

int main() {
  const char *what = "sweep";
  const int Ts[] = {15, 16, 17, 120, 121};
  const int rpP[][3] = {{4, 8, 16}, {5, 10, 16}, {8, 12, 16}, {13, 18, 32}};
  const double tols[] = {-1e-10, 1e-10};
  const double hmaxs[] = {1.0, 0.0, std::numeric_limits<double>::infinity()};
  const double spreads[] = {0.5, 1.6, 50.0};   // not warm, degree 6, degree 3
  const int maxits[] = {1, 2, 30};
  for (int bits = 0; bits < 64; ++bits) {
    FactSwitches sw;
    sw.keep_step0 = bits & 1;
    sw.f32_off = bits & 2;
    sw.split_off = bits & 4;
    sw.split_last_off = bits & 8;
    sw.pf_stored = !(bits & 16);
    sw.ap2_probe_off = bits & 32;
    for (int T : Ts)
      for (auto &g : rpP)
        for (double tol : tols)
          for (int hh = 0; hh < 4; ++hh)
            for (double hmax : hmaxs)
              for (double spread : spreads)
                for (int maxit : maxits)
                  for (int kwd = -1; kwd <= 0; ++kwd)        // kw below k, kw at least k
                    for (double lamk : {1.0, 0.0})
                      for (double fscale : {2.0, 0.0}) {
                        FilterPlanIn in;
                        in.warm = true;
                        in.r = g[0]; in.k = g[0]; in.p = g[1]; in.P = g[2];
                        in.kw = in.k + kwd;
                        in.T = T; in.maxit = maxit; in.tol = tol; in.spread = spread; in.lamk = lamk;
                        in.fscale = fscale; in.has_H32 = hh & 1; in.has_Hs = hh & 2; in.hmax = hmax;
                        check_plan(in, sw, what);
                      }
  }
  // the degrees the sweep is meant to reach, and a cold start
  CHECK(first_filter_degree(1.6, kChebWarmD0) == 6 && first_filter_degree(50.0, kChebWarmD0) == 3);
  {
    FilterPlanIn in;
    in.r = in.k = 8; in.p = 12; in.T = 120; in.maxit = 30; in.tol = -1e-10; in.spread = 1.6; in.lamk = 1.0;
    in.has_H32 = in.has_Hs = true; in.hmax = 1.0;
    check_plan(in, FactSwitches{}, "cold");
  }

  // three broken chains, each one edit away from a plan of the sweep
  FilterPlanIn in;
  in.warm = true; in.r = in.k = in.kw = 8; in.p = 12; in.T = 121; in.maxit = 30; in.tol = -1e-10; in.spread = 1.6;
  in.lamk = 1.0; in.fscale = 2.0; in.has_H32 = in.has_Hs = true; in.hmax = 1.0;
  FactSwitches last_off;
  last_off.split_last_off = true;
  const FilterPlan all_split = plan_first_filter(in, FactSwitches{}), fp64_last = plan_first_filter(in, last_off);
  what = "broken";
  CHECK(all_split.consistent() && all_split.d0 == 6 && all_split.product[6] == HzProduct::SplitRows);
  CHECK(fp64_last.consistent() && fp64_last.product[6] == HzProduct::F64 && fp64_last.mid_out[5] == ZFmt::F64);
  {   // a Split product behind an F32 Z
    FilterPlan b = all_split;
    b.mid_out[2] = ZFmt::F32;
    CHECK(b.product[3] == HzProduct::Split && !b.consistent());
  }
  {   // an F64 product behind Split planes
    FilterPlan b = fp64_last;
    b.mid_out[5] = ZFmt::Split;
    CHECK(b.product[6] == HzProduct::F64 && !b.consistent());
  }
  {   // a last Horner step behind Chunk32
    FilterPlan b = all_split;
    b.product[6] = HzProduct::Split;
    CHECK(result_of(b.product[6]) == HzFmt::Chunk32 && !b.consistent());
  }
  {   // (and the fp64 Z's pad rows left unwritten)
    FilterPlan b = all_split;
    CHECK(b.zero_zpad);
    b.zero_zpad = false;
    CHECK(!b.consistent());
  }
  if (failures) {
    std::printf("%ld failures in %ld plans\n", failures, plans);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
