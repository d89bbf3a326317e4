// Stand-alone check of csrc/dfm_criteria.h with a plain C++ compiler: no HIP,
// nothing linked from the project.  Every input is an integer-valued or dyadic
// double, so every sum below is exact and every comparison is ==.
#include "dfm_criteria.h"

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
  // ---- ceil_half, odd and even
  CHECK(ceil_half(1) == 1 && ceil_half(2) == 1 && ceil_half(7) == 4 && ceil_half(8) == 4 && ceil_half(9) == 5);

  // ---- the sweep's table equals the single criterion at the same (V_k, k)
  const double ev[8] = {32.0, 16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 0.25};   // descending; sum 63.75
  const int shapes[3][2] = {{8, 16}, {16, 8}, {4, 32}};               // N T = 128: V_k exact
  for (const auto &sh : shapes) {
    const int64_t T = sh[0], N = sh[1];
    const double trace = 64.0, sigma2 = 0.375, NT = 128.0;
    for (int kmax = 1; kmax <= 8; ++kmax) {
      double tab[7 * 8];
      int arg[7];
      criteria_sweep(ev, kmax, trace, sigma2, T, N, tab, arg);
      for (int code = 0; code < 7; ++code) CHECK(arg[code] == first_argmin(tab + code * kmax, kmax));
      double top = 0.0;
      for (int k = 1; k <= kmax; ++k) {
        top += ev[k - 1];
        const double V = (trace - top) / NT;
        for (int code = 0; code < 7; ++code) CHECK(tab[code * kmax + k - 1] == criterion(code, V, k, sigma2, T, N));
      }
    }
  }
  {   // V reaching zero: log(V) = -inf in the ICp rows, still equal entry by entry
    const double e2[2] = {48.0, 16.0};
    double tab[14];
    criteria_sweep(e2, 2, 64.0, 0.5, 8, 16, tab);
    for (int code = 0; code < 7; ++code) CHECK(tab[code * 2 + 1] == criterion(code, 0.0, 2, 0.5, 8, 16));
  }

  // ---- first arg-min
  const double tie[5] = {3.0, 1.0, 2.0, 1.0, 5.0};
  CHECK(first_argmin(tie, 5) == 2);
  const double dec[5] = {5.0, 4.0, 3.0, 2.0, 1.0};
  CHECK(first_argmin(dec, 5) == 5);
  const double nan = NAN, nans[4] = {nan, nan, nan, nan};
  CHECK(first_argmin(nans, 4) == 1);
  CHECK(first_argmin(dec, 1) == 1);

  // ---- both sigma^2 forms against the closed form sum_{j >= ceil(m/2)} ev[j] / (N T)
  CHECK(sigma2_tail(ev, 8, 128.0) == 3.75 / 128.0);
  CHECK(sigma2_total_minus_top(ev, 8, 128.0) == 3.75 / 128.0);
  CHECK(sigma2_minus_top(63.75, ev, 8, 128.0) == 3.75 / 128.0);
  CHECK(sigma2_tail(ev, 7, 64.0) == 3.5 / 64.0);   // odd m: the top 4 of 7 leave
  CHECK(sigma2_total_minus_top(ev, 7, 64.0) == 3.5 / 64.0);
  CHECK(tail_sum(ev, 8, 0) == 63.75);

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
