// Stand-alone check of the split products' refinement in csrc/dfm_fact_plan.h
// (terms, z0_planes, mid_planes, products_split3) with a plain C++ compiler:
// no HIP, nothing linked from the project.  fact_plan_host.cpp holds the
// kernels and formats of every plan against the rule as it stood; this one
// sweeps the same inputs crossed with split3_off and holds the new fields
// against their statement: three terms exactly in the Split products sp <=
// d0 - 2 with the switch on, six in every other split product, none elsewhere;
// every Split Z written with the planes its product reads; the counter; and
// the old fields untouched by the switch.  Every plan must be consistent(),
// and plans broken by hand to three terms behind three planes, or six behind
// two, must not be.
#include "dfm_fact_plan.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

using namespace dfm;

static long failures = 0, plans = 0, three_term_plans = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (failures < 20) std::printf("FAILED line %d (%s): %s\n", __LINE__, what, #cond); \
      ++failures;                                                                \
    }                                                                            \
  } while (0)

static bool is_split(HzProduct k) { return k == HzProduct::Split || k == HzProduct::SplitRows; }

static void check_plan(const FilterPlanIn &in, const FactSwitches &sw, const char *what) {
  const FilterPlan pl = plan_first_filter(in, sw);
  ++plans;
  CHECK(pl.consistent());
  int n3 = 0;
  for (int sp = 1; sp <= pl.d0; ++sp) {
    const bool three = pl.product[sp] == HzProduct::Split && sp <= pl.d0 - 2 && !sw.split3_off;
    CHECK(pl.terms[sp] == (three ? 3 : is_split(pl.product[sp]) ? 6 : 0));
    n3 += three;
    // planes written (by prep, or by the middle step in front) equal planes read
    const int written = sp == 1 ? pl.z0_planes : pl.mid_planes[sp - 1];
    const ZFmt zin = sp == 1 ? pl.z0 : pl.mid_out[sp - 1];
    CHECK(written == (zin != ZFmt::Split ? 0 : pl.terms[sp] == 3 ? 2 : 3));
    CHECK((zin == ZFmt::Split) == is_split(pl.product[sp]));
  }
  for (int sp = pl.d0 + 1; sp <= kFilterDMax; ++sp) CHECK(pl.terms[sp] == 0);
  for (int sp = pl.d0; sp <= kFilterDMax; ++sp) CHECK(pl.mid_planes[sp] == 0);
  CHECK(pl.products_split3 == n3);
  CHECK(pl.products_split3 <= pl.products_f32);
  const bool all_split = pl.product[1] == HzProduct::Split;
  CHECK(pl.products_split3 == (all_split && !sw.split3_off ? pl.d0 - 2 : 0));
  three_term_plans += n3 > 0;
  // the switch moves nothing but the new fields
  FactSwitches other = sw;
  other.split3_off = !sw.split3_off;
  const FilterPlan po = plan_first_filter(in, other);
  CHECK(po.d0 == pl.d0 && po.warm_started == pl.warm_started && po.mid == pl.mid && po.skip0 == pl.skip0 &&
        po.nopf == pl.nopf && po.stg_ok == pl.stg_ok && po.z0 == pl.z0 && po.pad_rows == pl.pad_rows &&
        po.zero_zpad == pl.zero_zpad && po.products_f32 == pl.products_f32 &&
        po.products_split_last == pl.products_split_last);
  for (int sp = 1; sp <= pl.d0; ++sp) {
    CHECK(po.product[sp] == pl.product[sp]);
    if (sp < pl.d0) CHECK(po.mid_in[sp] == pl.mid_in[sp] && po.mid_out[sp] == pl.mid_out[sp]);
  }
}

int main() {
  const char *what = "sweep";
  const int Ts[] = {15, 16, 17, 120, 121};
  const int rpP[][3] = {{4, 8, 16}, {5, 10, 16}, {8, 12, 16}, {13, 18, 32}};
  const double tols[] = {-1e-10, 1e-10};
  const double hmaxs[] = {1.0, 0.0, std::numeric_limits<double>::infinity()};
  const double spreads[] = {0.5, 1.6, 50.0};   // not warm, degree 6, degree 3
  const int maxits[] = {1, 2, 30};
  for (int bits = 0; bits < 128; ++bits) {
    FactSwitches sw;
    sw.keep_step0 = bits & 1;
    sw.f32_off = bits & 2;
    sw.split_off = bits & 4;
    sw.split_last_off = bits & 8;
    sw.pf_stored = !(bits & 16);
    sw.ap2_probe_off = bits & 32;
    sw.split3_off = bits & 64;
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
  CHECK(three_term_plans > 0);
  {
    FilterPlanIn in;   // a cold start
    in.r = in.k = 8; in.p = 12; in.T = 120; in.maxit = 30; in.tol = -1e-10; in.spread = 1.6; in.lamk = 1.0;
    in.has_H32 = in.has_Hs = true; in.hmax = 1.0;
    check_plan(in, FactSwitches{}, "cold");
  }

  // the production plans, spelled out: degree 6 and degree 3, switch on and off, fp64 last product
  FilterPlanIn in;
  in.warm = true; in.r = in.k = in.kw = 8; in.p = 12; in.T = 121; in.maxit = 30; in.tol = -1e-10; in.spread = 1.6;
  in.lamk = 1.0; in.fscale = 2.0; in.has_H32 = in.has_Hs = true; in.hmax = 1.0;
  what = "spelled out";
  const FilterPlan d6 = plan_first_filter(in, FactSwitches{});
  {
    const int want[7] = {0, 3, 3, 3, 3, 6, 6}, planes[6] = {0, 2, 2, 2, 3, 3};
    CHECK(d6.d0 == 6 && d6.products_split3 == 4 && d6.products_f32 == 5 && d6.products_split_last == 1);
    CHECK(d6.z0_planes == 2);
    for (int sp = 1; sp <= 6; ++sp) CHECK(d6.terms[sp] == want[sp]);
    for (int sp = 1; sp < 6; ++sp) CHECK(d6.mid_planes[sp] == planes[sp]);
  }
  {
    FactSwitches off;
    off.split3_off = true;
    const FilterPlan b = plan_first_filter(in, off);
    CHECK(b.products_split3 == 0 && b.z0_planes == 3 && b.products_f32 == 5);
    for (int sp = 1; sp <= 6; ++sp) CHECK(b.terms[sp] == 6);
    for (int sp = 1; sp < 6; ++sp) CHECK(b.mid_planes[sp] == 3);
  }
  {
    FactSwitches last_off;
    last_off.split_last_off = true;
    const FilterPlan b = plan_first_filter(in, last_off);
    CHECK(b.consistent() && b.products_split3 == 4 && b.terms[5] == 6 && b.terms[6] == 0 && b.mid_planes[4] == 3 &&
          b.mid_planes[5] == 0);
  }
  {
    FilterPlanIn c2 = in;
    c2.spread = 50.0;
    const FilterPlan b = plan_first_filter(c2, FactSwitches{});
    CHECK(b.d0 == 3 && b.products_split3 == 1 && b.terms[1] == 3 && b.terms[2] == 6 && b.terms[3] == 6 &&
          b.z0_planes == 2 && b.mid_planes[1] == 3 && b.mid_planes[2] == 3);
  }

  // broken by hand, each one edit away from the production plan
  what = "broken";
  CHECK(d6.consistent());
  {   // three terms behind three planes (a middle step)
    FilterPlan b = d6;
    b.mid_planes[2] = 3;
    CHECK(b.terms[3] == 3 && !b.consistent());
  }
  {   // three terms behind three planes (prep)
    FilterPlan b = d6;
    b.z0_planes = 3;
    CHECK(b.terms[1] == 3 && !b.consistent());
  }
  {   // three terms where the writer was left at three planes
    FilterPlan b = d6;
    b.terms[5] = 3;
    CHECK(b.mid_planes[4] == 3 && !b.consistent());
  }
  {   // six terms behind two planes
    FilterPlan b = d6;
    b.terms[3] = 6;
    CHECK(b.mid_planes[2] == 2 && !b.consistent());
  }
  {   // six terms behind two planes (the last product)
    FilterPlan b = d6;
    b.mid_planes[5] = 2;
    CHECK(b.terms[6] == 6 && !b.consistent());
  }
  {   // a term count that no kernel has
    FilterPlan b = d6;
    b.terms[2] = 1;
    CHECK(!b.consistent());
  }
  if (failures) {
    std::printf("%ld failures in %ld plans\n", failures, plans);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
