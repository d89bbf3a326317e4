// Stand-alone check of the mixed-frequency host functions in
// csrc/dfm_ss_host.h with a plain C++ compiler: the limits and the checks of
// the weights, the padded companion matrix, Z_l, the stationary covariance at
// the padded state, and the fit's start values of the low series.  No HIP,
// nothing linked from the project.
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
  const double flow[5] = {1.0, 2.0, 3.0, 2.0, 1.0};
  const uint8_t low[4] = {0, 0, 1, 1}, none[4] = {0, 0, 0, 0};
  // ---- the lag count and the limits at the padded state
  CHECK(ss_mf_lags(1, 5) == 5 && ss_mf_lags(8, 5) == 8 && ss_mf_lags(3, 3) == 3);
  CHECK(ss_mf_check(2, 1, 5, flow, low) == 0);
  CHECK(ss_mf_check(6, 1, 5, flow, low) == 0);                 // s = 30
  CHECK(ss_mf_check(8, 1, 5, flow, low) == SS_E_LIMIT);        // s = 40
  CHECK(ss_mf_check(4, 8, 5, flow, low) == 0);                 // s = 32 with L = p
  CHECK(ss_mf_check(4, 9, 5, flow, low) == SS_E_LIMIT);
  CHECK(ss_mf_check(17, 1, 1, flow, low) == SS_E_LIMIT);
  CHECK(ss_mf_check(2, 1, 9, flow, low) == SS_E_LIMIT);        // n_w beyond 8, before w is read
  CHECK(ss_mf_check(2, 1, 0, flow, low) == -2);
  CHECK(ss_mf_check(0, 1, 5, flow, low) == -2);
  CHECK(ss_mf_check(2, 0, 5, flow, low) == -2);
  // ---- the weights and the mask
  CHECK(ss_mf_check(2, 1, 5, nullptr, low) == -2);
  CHECK(ss_mf_check(2, 1, 5, flow, nullptr) == -2);
  double w[3] = {1.0, NAN, 1.0};
  CHECK(ss_mf_check(2, 1, 3, w, low) == -2);
  CHECK(ss_mf_check(2, 1, 1, w, low) == 0);                    // the NaN lies beyond n_w
  w[1] = INFINITY;
  CHECK(ss_mf_check(2, 1, 3, w, low) == -2);
  w[0] = 0.0, w[1] = 1.0;
  CHECK(ss_mf_check(2, 1, 3, w, low) == -2);                   // w_0 = 0
  w[0] = -0.5;
  CHECK(ss_mf_check(2, 1, 3, w, low) == 0);                    // a negative weight is a weight
  CHECK(ss_mf_any_low(low, 4) && !ss_mf_any_low(low, 2) && !ss_mf_any_low(none, 4));
  // ---- [A 0] and its companion matrix: r = 2, p = 1, L = 3
  const double A[4] = {0.5, 0.1, -0.2, 0.4};   // column-major: A = [0.5 -0.2; 0.1 0.4]
  double Apad[12], Tm[36];
  ss_mf_pad_A(A, 2, 1, 3, Apad);
  for (int e = 0; e < 12; ++e) CHECK(Apad[e] == (e < 4 ? A[e] : 0.0));
  ss_companion(Apad, 2, 3, Tm);
  const double want[36] = {0.5, -0.2, 0, 0, 0, 0,  0.1, 0.4, 0, 0, 0, 0,  1, 0, 0, 0, 0, 0,
                           0,   1,    0, 0, 0, 0,  0,   0,   1, 0, 0, 0,  0, 0, 0, 1, 0, 0};
  for (int e = 0; e < 36; ++e) CHECK(Tm[e] == want[e]);
  ss_mf_pad_A(A, 2, 1, 1, Apad);               // L = p: A itself
  for (int e = 0; e < 4; ++e) CHECK(Apad[e] == A[e]);
  // ---- Z_l: r = 2, s = 8, three weights
  const double w3[3] = {1.0, 2.0, 3.0};
  double Zl[16];
  ss_mf_zl(w3, 3, 2, 8, Zl);
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 8; ++j) CHECK(Zl[i * 8 + j] == ((j % 2 == i && j < 6) ? w3[j / 2] : 0.0));
  // ---- the stationary covariance of the padded form: its leading block is the
  // unpadded one's, and the lag blocks on the diagonal repeat it (a scalar AR(1):
  // P[k][k] = q / (1 - a^2), P[0][k] = a^k P[0][0])
  const double a1[3] = {0.5, 0.0, 0.0}, q1[1] = {0.75};
  double P1[1], P3[9];
  CHECK(ss_stationary_cov(a1, q1, 1, 1, P1) == 0 && ss_stationary_cov(a1, q1, 1, 3, P3) == 0);
  CHECK(fabs(P1[0] - 1.0) < 1e-15);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) CHECK(fabs(P3[i * 3 + j] - pow(0.5, abs(i - j))) < 1e-15);

  // ---- the low series' start values: T = 8, N = 2, r = 1, w = (1, 1); column 1 is low with
  // z_t = 2 (F_t + F_{t-1}) on its observed rows, an exact fit at first
  {
    const double F[8] = {1, 2, 4, 3, 5, 8, 6, 7}, w2[2] = {1.0, 1.0};
    const uint8_t lo[2] = {0, 1};
    double Zm[16], L[2] = {9.0, 9.0}, sg[2] = {9.0, 9.0};
    for (int t = 0; t < 8; ++t) Zm[t] = 1.0, Zm[8 + t] = t >= 1 ? 2.0 * (F[t] + F[t - 1]) : 100.0;   // row 0 is not used
    Zm[8 + 3] = NAN;
    int64_t where = -1;
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 1, w2, 2, lo, L, sg, &where) == SS_E_SIGMA && where == 1);   // an exact fit
    CHECK(L[0] == 9.0 && sg[0] == 9.0);
    // ft on the used rows 1, 2, 4..7 is 3, 6, 8, 13, 14, 13; with a residual at rows 2 and 4 the
    // result is the scalar regression's
    Zm[8 + 2] += 1.0, Zm[8 + 4] -= 1.0;
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 1, w2, 2, lo, L, sg, &where) == 0 && L[0] == 9.0 && sg[0] == 9.0);
    const double ft[6] = {3, 6, 8, 13, 14, 13}, z[6] = {6, 13, 15, 26, 28, 26};
    double num = 0.0, den = 0.0, rss = 0.0;
    for (int k = 0; k < 6; ++k) num += ft[k] * z[k], den += ft[k] * ft[k];
    for (int k = 0; k < 6; ++k) rss += (z[k] - num / den * ft[k]) * (z[k] - num / den * ft[k]);
    CHECK(fabs(L[1] - num / den) < 1e-15 && fabs(sg[1] - rss / 6.0) < 1e-15);
    for (int t = 3; t < 8; ++t) Zm[8 + t] = NAN;   // rows 1, 2 left: r + 1 = 2 rows are enough, one is not
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 1, w2, 2, lo, L, sg, &where) == 0);
    Zm[8 + 2] = NAN;
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 1, w2, 2, lo, L, sg, &where) == SS_E_VAR && where == 1);
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 1, w2, 9, lo, L, sg, &where) == -2);
    CHECK(ss_mf_start(nullptr, 8, 2, 8, F, 1, w2, 2, lo, L, sg, &where) == -2);
  }

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
