// Stand-alone check of the host functions of the AR(1) idiosyncratic terms in
// csrc/dfm_ss_host.h with a plain C++ compiler: the limits and the checks of
// rho, the two-step estimate with its clamp and its fallback, and the fill
// rule's three cases.  Hand-worked cases, checked as equalities (1e-15 where a
// quotient is not a binary fraction).  No HIP, nothing linked from the project.
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
  // ---- the lag count and the limits at the padded state
  CHECK(ss_ar_lags(1) == 2 && ss_ar_lags(2) == 2 && ss_ar_lags(3) == 3);
  const double ok[3] = {0.5, 0.0, -0.9};
  int64_t where = 7;
  CHECK(ss_ar_check(8, 4, 3, ok, &where) == 0 && where == -1);   // ru = 16, s = 32
  CHECK(ss_ar_check(8, 1, 3, ok, &where) == 0);                  // s = 16 at L = 2
  CHECK(ss_ar_check(9, 1, 3, ok, &where) == SS_E_LIMIT);         // ru = 18
  CHECK(ss_ar_check(8, 5, 3, ok, &where) == SS_E_LIMIT);         // s = 40
  CHECK(ss_ar_check(4, 8, 3, ok, &where) == 0);
  CHECK(ss_ar_check(4, 9, 3, ok, &where) == SS_E_LIMIT);
  CHECK(ss_ar_check(0, 1, 3, ok, &where) == -2);
  CHECK(ss_ar_check(2, 0, 3, ok, &where) == -2);
  CHECK(ss_ar_check(2, 1, 0, ok, &where) == -2);
  CHECK(ss_ar_check(9, 1, 3, nullptr, &where) == SS_E_LIMIT);    // the limits before rho is read
  // ---- rho
  CHECK(ss_ar_check(2, 1, 3, nullptr, &where) == -2 && where == -1);
  double rho[3] = {0.5, 1.0, 0.0};
  CHECK(ss_ar_check(2, 1, 3, rho, &where) == -2 && where == 1);
  rho[1] = 0.0, rho[2] = -1.0;
  CHECK(ss_ar_check(2, 1, 3, rho, &where) == -2 && where == 2);
  rho[2] = INFINITY;
  CHECK(ss_ar_check(2, 1, 3, rho, &where) == -2 && where == 2);
  rho[0] = 1.0, rho[2] = NAN;
  CHECK(ss_ar_check(2, 1, 3, rho, &where) == SS_E_NAN);          // NaN anywhere comes first
  CHECK(ss_ar_check(2, 1, 2, rho, &where) == -2 && where == 0);  // the NaN lies beyond N
  CHECK(ss_ar_check(2, 1, 3, ok, nullptr) == 0);

  // ---- the estimate: r = 1, F = 0, so eps = Zm.  T = 5, six series:
  //   0: eps = 2 1 1 0 -1    num 3, den 6: rho = 1/2; u = 0 .5 -.5 -1: sigma2 = 1.5 / 4
  //   1: eps = 1 2 4 8 16    num 170, den 85: rho = 2, clamped to 0.99
  //   2: eps = 1 -2 4 -8 16  rho = -2, clamped to -0.99
  //   3: eps = 1 2 . 3 4     two pairs: rho = 0, sigma2 as it came
  //   4: eps = 0 0 0 0 1     a zero denominator: rho = 0, sigma2 as it came
  //   5: eps = . 1 3 5 9     three pairs: num 3 + 15 + 45 = 63, den 1 + 9 + 25 = 35: rho = 1.8 -> 0.99
  const int T = 5, N = 6;
  const double Zm[T * N] = {2, 1, 1, 0, -1, 1, 2, 4, 8, 16, 1, -2, 4, -8, 16, 1, 2, NAN, 3, 4, 0, 0, 0, 0, 1, NAN, 1, 3, 5, 9};
  const double F[T] = {0, 0, 0, 0, 0}, L[N] = {1, 1, 1, 1, 1, 1};
  double sig[N] = {7, 7, 7, 7, 7, 7}, rh[N] = {9, 9, 9, 9, 9, 9};
  CHECK(ss_ar_estimate(Zm, T, N, T, F, L, 1, sig, rh, &where) == 0);
  CHECK(rh[0] == 0.5 && sig[0] == 0.375);
  CHECK(rh[1] == SS_AR_RHO_MAX && rh[1] == 0.99);
  {
    double ss = 0.0;
    const double e[5] = {1, 2, 4, 8, 16};
    for (int t = 1; t < 5; ++t) ss += (e[t] - 0.99 * e[t - 1]) * (e[t] - 0.99 * e[t - 1]);
    CHECK(fabs(sig[1] - ss / 4.0) <= 1e-15 * ss);
  }
  CHECK(rh[2] == -0.99 && fabs(sig[2] - sig[1]) <= 1e-15 * sig[1]);
  CHECK(rh[3] == 0.0 && sig[3] == 7.0);
  CHECK(rh[4] == 0.0 && sig[4] == 7.0);
  CHECK(rh[5] == 0.99);
  // a variance that stays non-positive is refused, with its column
  sig[3] = 0.0;
  CHECK(ss_ar_estimate(Zm, T, N, T, F, L, 1, sig, rh, &where) == SS_E_SIGMA && where == 3);
  // an exact AR(1) path leaves no innovation: -10 as well
  {
    const double Zg[5] = {1, 0.5, 0.25, 0.125, 0.0625};
    double s1[1] = {1.0}, r1[1];
    CHECK(ss_ar_estimate(Zg, 5, 1, 5, F, L, 1, s1, r1, &where) == SS_E_SIGMA && where == 0 && r1[0] == 0.5);
  }
  // ---- steps 2-4 together: P0 is that of the padded state, s = r max(p, 2) = 2
  {
    const int Te = 12;
    const double Fe[Te] = {1, -1, 2, -2, 1, 0, -1, 2, 1, -2, 0, 1};
    double Ze[Te * 2];
    for (int t = 0; t < Te; ++t) Ze[t] = Fe[t] + ((t * 5) % 3 - 1.0), Ze[Te + t] = -Fe[t] + ((t * 7) % 4 - 1.5);
    const double Le[2] = {1.0, -1.0};
    double s2[2], A[1], Q[1], P0[4], r2[2];
    CHECK(ss_estimate_ar(Ze, Te, 2, Te, Fe, Le, 1, 1, s2, A, Q, P0, r2, &where) == 0);
    CHECK(fabs(A[0]) < 1.0 && Q[0] > 0.0 && s2[0] > 0.0 && s2[1] > 0.0 && fabs(r2[0]) <= 0.99 && fabs(r2[1]) <= 0.99);
    const double v = Q[0] / (1.0 - A[0] * A[0]);   // f_t and f_{t-1} share the stationary variance
    CHECK(fabs(P0[0] - v) <= 1e-14 * v && fabs(P0[3] - v) <= 1e-14 * v);
    CHECK(P0[1] == P0[2] && fabs(P0[1] - A[0] * v) <= 1e-14 * v);
    CHECK(ss_estimate_ar(Ze, Te, 2, Te, Fe, Le, 9, 1, s2, A, Q, P0, r2, &where) == SS_E_LIMIT);
    CHECK(ss_estimate_ar(Ze, Te, 2, Te, Fe, Le, 1, 1, s2, A, Q, P0, nullptr, &where) == -2);
  }

  // ---- the fill: T = 6, h = 2, r = 1, lambda = 2, f_t|T = 1: the common component is 2
  //   0 (rho 1/2): . . 6 3 3 10   late starter, ehat_v = 4: rows 1, 0 -> 2 + 2, 2 + 1;
  //                               forecast, ehat_u = 8: rows 6, 7 -> 2 + 4, 2 + 2
  //   1 (rho 1/2): 3 . . 4 5 .    bridge u = 0 (ehat 1), v = 3 (ehat 2): rows 1, 2 -> 2 + 6/7, 2 + 8/7;
  //                               ragged edge, ehat_u = 3: rows 5, 6, 7 -> 2 + 3/2, 2 + 3/4, 2 + 3/8
  //   2 (rho 0):   3 . . 4 5 .    every missing entry is the common component
  //   3 (rho 1/2): all missing    the common component
  //   4 (rho -1/2): 4 . 4 4 4 4   bridge d1 = d2 = 1, ehat 2 and 2: e = -1/2 (3/4) 4 / (15/16) = -8/5; forecast 2 - 1, 2 + 1/2
  {
    const int Tf = 6, h = 2, Nf = 5, Tt = Tf + h;
    const double X[Tf * Nf] = {NAN, NAN, 6, 3, 3, 10, 3, NAN, NAN, 4, 5, NAN, 3, NAN, NAN, 4, 5, NAN,
                               NAN, NAN, NAN, NAN, NAN, NAN, 4, NAN, 4, 4, 4, 4};
    const double Lf[Nf] = {2, 2, 2, 2, 2}, rf[Nf] = {0.5, 0.5, 0.0, 0.5, -0.5};
    double S[Tt], out[Tt * Nf];
    for (int t = 0; t < Tt; ++t) S[t] = 1.0;
    ss_ar_fill(X, Tf, Nf, Tf, Lf, 1, rf, S, h, out);
    const double *o = out;
    CHECK(o[0] == 3.0 && o[1] == 4.0 && o[2] == 6.0 && o[3] == 3.0 && o[4] == 3.0 && o[5] == 10.0 && o[6] == 6.0 && o[7] == 4.0);
    o = out + Tt;
    CHECK(o[0] == 3.0 && o[3] == 4.0 && o[4] == 5.0);
    CHECK(fabs(o[1] - (2.0 + 6.0 / 7.0)) <= 1e-15 && fabs(o[2] - (2.0 + 8.0 / 7.0)) <= 1e-15);
    CHECK(o[5] == 3.5 && o[6] == 2.75 && o[7] == 2.375);
    o = out + 2 * Tt;
    CHECK(o[0] == 3.0 && o[1] == 2.0 && o[2] == 2.0 && o[3] == 4.0 && o[4] == 5.0 && o[5] == 2.0 && o[6] == 2.0 && o[7] == 2.0);
    o = out + 3 * Tt;
    for (int t = 0; t < Tt; ++t) CHECK(o[t] == 2.0);
    o = out + 4 * Tt;
    CHECK(o[0] == 4.0 && fabs(o[1] - (2.0 - 1.6)) <= 1e-15 && o[2] == 4.0 && o[5] == 4.0 && o[6] == 1.0 && o[7] == 2.5);
    // a panel with a leading dimension, no forecast rows
    double Xl[2 * 4] = {1, NAN, 5, 99, NAN, 3, 3, 99}, out2[3 * 2];
    const double S3[3] = {1.0, 1.0, 1.0}, L2[2] = {1.0, 1.0}, r2[2] = {0.5, 0.5};
    ss_ar_fill(Xl, 3, 2, 4, L2, 1, r2, S3, 0, out2);
    CHECK(out2[0] == 1.0 && out2[2] == 5.0 && out2[3] == 2.0 && out2[4] == 3.0 && out2[5] == 3.0);
    CHECK(fabs(out2[1] - (1.0 + (0.5 * 0.75 * 0.0 + 0.5 * 0.75 * 4.0) / 0.9375)) <= 1e-15);
  }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
