// Stand-alone check of the news decomposition's host arithmetic in
// csrc/dfm_ss_host.h with a plain C++ compiler: no HIP, nothing linked from the
// project.  Every refusal of the release list with the entry it names, J = 0,
// the revised panel, the argument checks and the releases per pass.
#include "dfm_ss_host.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
      ++failures;                                              \
    }                                                          \
  } while (0)

int main() {
  using namespace dfm;
  // Two vintages of a 4 x 3 panel, column-major with ldx = 5 (the fifth row is
  // padding and must not be read as data: it holds a value in X_old only).
  // Releases: (1, 2), (3, 0), (3, 1).  (0, 0) is revised; (2, 1) is NaN in both.
  const int64_t T = 4, N = 3, ldx = 5;
  const double Xn[15] = {1.0, 2.0, 3.0, 4.0, NAN, 5.0, 6.0, NAN, 8.0, NAN, 9.0, 10.0, 11.0, 12.0, NAN};
  double Xo[15] = {1.5, 2.0, 3.0, NAN, 7.0, 5.0, 6.0, NAN, NAN, 7.0, 9.0, NAN, 11.0, 12.0, 7.0};
  int64_t bt = -9, bi = -9;
  auto check = [&](const double *xo, int64_t J, const int64_t *rt, const int64_t *ri) {
    bt = bi = -9;
    return ss_news_check_releases(xo, Xn, T, N, ldx, J, rt, ri, &bt, &bi);
  };
  {   // the exact list
    const int64_t rt[3] = {1, 3, 3}, ri[3] = {2, 0, 1};
    CHECK(check(Xo, 3, rt, ri) == SS_NEWS_OK);
  }
  {   // unsorted: by row, then by series within a row
    const int64_t rt[3] = {3, 1, 3}, ri[3] = {0, 2, 1};
    CHECK(check(Xo, 3, rt, ri) == SS_NEWS_UNSORTED && bt == 1 && bi == 2);
    const int64_t rt2[3] = {1, 3, 3}, ri2[3] = {2, 1, 0};
    CHECK(check(Xo, 3, rt2, ri2) == SS_NEWS_UNSORTED && bt == 3 && bi == 0);
  }
  {   // duplicate
    const int64_t rt[4] = {1, 3, 3, 3}, ri[4] = {2, 0, 0, 1};
    CHECK(check(Xo, 4, rt, ri) == SS_NEWS_DUPLICATE && bt == 3 && bi == 0);
  }
  {   // missing one: the first, one in the middle, the last
    const int64_t rt[2] = {3, 3}, ri[2] = {0, 1};
    CHECK(check(Xo, 2, rt, ri) == SS_NEWS_MISSING && bt == 1 && bi == 2);
    const int64_t rt2[2] = {1, 3}, ri2[2] = {2, 1};
    CHECK(check(Xo, 2, rt2, ri2) == SS_NEWS_MISSING && bt == 3 && bi == 0);
    const int64_t rt3[2] = {1, 3}, ri3[2] = {2, 0};
    CHECK(check(Xo, 2, rt3, ri3) == SS_NEWS_MISSING && bt == 3 && bi == 1);
  }
  {   // not a release: observed in both, NaN in both
    const int64_t rt[4] = {0, 1, 3, 3}, ri[4] = {0, 2, 0, 1};
    CHECK(check(Xo, 4, rt, ri) == SS_NEWS_NOT_NEW && bt == 0 && bi == 0);
    const int64_t rt2[4] = {1, 2, 3, 3}, ri2[4] = {2, 1, 0, 1};
    CHECK(check(Xo, 4, rt2, ri2) == SS_NEWS_NOT_NEW && bt == 2 && bi == 1);
  }
  {   // outside the panel (row T is the padding row)
    const int64_t rt[3] = {1, 3, 4}, ri[3] = {2, 0, 1};
    CHECK(check(Xo, 3, rt, ri) == SS_NEWS_RANGE && bt == 4 && bi == 1);
    const int64_t rt2[1] = {1}, ri2[1] = {3};
    CHECK(check(Xo, 1, rt2, ri2) == SS_NEWS_RANGE && bt == 1 && bi == 3);
    const int64_t rt3[1] = {-1}, ri3[1] = {0};
    CHECK(check(Xo, 1, rt3, ri3) == SS_NEWS_RANGE && bt == -1 && bi == 0);
  }
  {   // old not within new: (2, 1) observed in X_old only
    const int64_t rt[3] = {1, 3, 3}, ri[3] = {2, 0, 1};
    double Xd[15];
    for (int e = 0; e < 15; ++e) Xd[e] = Xo[e];
    Xd[1 * ldx + 2] = 4.5;
    CHECK(check(Xd, 3, rt, ri) == SS_NEWS_DROPPED && bt == 2 && bi == 1);
  }
  {   // J = 0: valid when the masks agree, a missing release otherwise; the lists are not read
    double Xs[15];
    for (int e = 0; e < 15; ++e) Xs[e] = Xn[e];
    Xs[0] = -1.0;   // a revision alone
    CHECK(check(Xs, 0, nullptr, nullptr) == SS_NEWS_OK);
    CHECK(check(Xo, 0, nullptr, nullptr) == SS_NEWS_MISSING && bt == 1 && bi == 2);
  }
  {   // the revised panel: X_new's values on the old observed set, ld T
    double Xr[12];
    ss_news_revised(Xo, Xn, T, N, ldx, Xr);
    const double want[12] = {1.0, 2.0, 3.0, NAN, 5.0, 6.0, NAN, NAN, 9.0, NAN, 11.0, 12.0};
    for (int e = 0; e < 12; ++e) CHECK(isnan(want[e]) ? isnan(Xr[e]) : Xr[e] == want[e]);
  }
  // ---- the call's own arguments
  CHECK(ss_news_check_args(3, true, 10, 2, 0, 0) == 0 && ss_news_check_args(0, false, 10, 0, 9, 64) == 0);
  CHECK(ss_news_check_args(3, true, 10, 2, 11, 0) == 0 && ss_news_check_args(3, true, 10, 2, 12, 0) == -2);
  CHECK(ss_news_check_args(3, false, 10, 0, 0, 0) == -2 && ss_news_check_args(-1, true, 10, 0, 0, 0) == -2);
  CHECK(ss_news_check_args(SS_NEWS_JMAX, true, 10, 0, 0, 0) == 0 && ss_news_check_args(SS_NEWS_JMAX + 1, true, 10, 0, 0, 0) == -2);
  CHECK(ss_news_check_args(3, true, 10, -1, 0, 0) == -2 && ss_news_check_args(3, true, 10, (1 << 20) + 1, 0, 0) == -2);
  CHECK(ss_news_check_args(3, true, 10, 0, -1, 0) == -2 && ss_news_check_args(3, true, 10, 0, 0, -1) == -2);
  CHECK(ss_news_check_args(3, true, 0, 0, 0, 0) == -2);
  // ---- releases per pass: a caller's cap, J below the rule, the rule in whole waves, one release too large
  CHECK(ss_news_releases_per_pass(72, 0, 2, 10, true, 492, 64) == 64);
  CHECK(ss_news_releases_per_pass(72, 0, 2, 10, true, 9, 64) == 9);
  CHECK(ss_news_releases_per_pass(72, 0, 2, 10, true, 492, 0) == 492);
  {   // Tt = 4096, r = 16, s = 32, t_lo = 0: 8 (4096 32 + 4 4096 16 + 17) = 3145864 bytes -> 170 -> 128
    CHECK(ss_news_releases_per_pass(4096, 0, 16, 32, true, 1000, 0) == 128);
    // plain: 8 (4096 32 + 2 4096 16 + 17) = 2097288 -> 255 -> 192; t_lo = 4095: 8 (131072 + 32 + 17) -> 511 -> 448
    CHECK(ss_news_releases_per_pass(4096, 0, 16, 32, false, 1000, 0) == 192);
    CHECK(ss_news_releases_per_pass(4096, 4095, 16, 32, false, 1000, 0) == 448);
    CHECK(ss_news_releases_per_pass(4096, 0, 16, 32, true, 100, 0) == 100);
  }
  CHECK(ss_news_releases_per_pass(((int64_t)1 << 20) + ((int64_t)1 << 24), 0, 16, 32, true, 5, 0) == 1);
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
