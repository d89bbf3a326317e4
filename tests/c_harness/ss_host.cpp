// Stand-alone check of csrc/dfm_ss_host.h with a plain C++ compiler: no HIP,
// nothing linked from the project.  Every input is an integer-valued or dyadic
// double, so every product and sum below is exact and every comparison is ==.
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
  // ---- the limits
  CHECK(ss_check_dims(1, 1) == 0 && ss_check_dims(16, 2) == 0 && ss_check_dims(4, 8) == 0 && ss_check_dims(8, 4) == 0);
  CHECK(ss_check_dims(17, 1) == SS_E_LIMIT && ss_check_dims(1, 9) == SS_E_LIMIT && ss_check_dims(12, 3) == SS_E_LIMIT);
  CHECK(ss_check_dims(0, 1) == -2 && ss_check_dims(1, 0) == -2);

  // ---- the companion form of r = 2, p = 3: A column-major 2 x 6
  const int r = 2, p = 3, s = 6;
  double A[12];
  for (int c = 0; c < s; ++c)
    for (int i = 0; i < r; ++i) A[c * r + i] = 0.125 * (1 + i) - 0.0625 * c;   // dyadic
  double Tm[36];
  ss_companion(A, r, p, Tm);
  for (int i = 0; i < s; ++i)
    for (int j = 0; j < s; ++j) {
      const double want = i < r ? A[j * r + i] : (j == i - r ? 1.0 : 0.0);
      CHECK(Tm[i * s + j] == want);
    }

  // ---- one doubling step, r = 2, p = 1: P + M P M' and M M by hand
  double M[4] = {0.5, 0.25, 0.0, -0.5}, P[4] = {2.0, 1.0, 1.0, 4.0}, W[8];
  ss_doubling_step(P, M, 2, W);
  // M P = [[1.25, 1.5], [-0.5, -2]];  M P M' = [[1, -0.75], [-0.75, 1]]
  CHECK(P[0] == 3.0 && P[1] == 0.25 && P[2] == 0.25 && P[3] == 5.0);
  CHECK(M[0] == 0.25 && M[1] == 0.0 && M[2] == 0.0 && M[3] == 0.25);

  // ---- the stationary covariance of a diagonal AR(1): q / (1 - a^2), a = 1/2 -> 4/3 q (not dyadic: a tolerance of
  //      one ulp), the symmetry exact; an explosive and a unit-root VAR, NaN and the limits are rejected
  const double Ad[4] = {0.5, 0.0, 0.0, 0.5}, Qd[4] = {3.0, 0.0, 0.0, 6.0};
  double P0[4];
  CHECK(ss_stationary_cov(Ad, Qd, 2, 1, P0) == 0);
  CHECK(fabs(P0[0] - 4.0) <= 1e-15 * 4.0 && fabs(P0[3] - 8.0) <= 1e-15 * 8.0 && P0[1] == 0.0 && P0[2] == 0.0);
  const double Ax[1] = {1.5}, Au[1] = {1.0}, Q1[1] = {1.0}, An[1] = {NAN};
  double p1[1];
  CHECK(ss_stationary_cov(Ax, Q1, 1, 1, p1) == SS_E_EXPLOSIVE);
  CHECK(ss_stationary_cov(Au, Q1, 1, 1, p1) == SS_E_EXPLOSIVE);
  CHECK(ss_stationary_cov(An, Q1, 1, 1, p1) == SS_E_NAN);
  CHECK(ss_stationary_cov(Ax, Q1, 17, 1, p1) == SS_E_LIMIT);
  CHECK(ss_stationary_cov(Ax, Q1, 12, 3, p1) == SS_E_LIMIT);

  // ---- the parameter checks
  const double L[4] = {1.0, 2.0, 3.0, 4.0};   // N = 2, r = 2
  double sg[2] = {1.0, 0.0};
  int64_t where = -1;
  CHECK(ss_check_params(2, 2, 1, L, sg, Ad, Qd, nullptr, nullptr, &where) == SS_E_SIGMA && where == 1);
  sg[1] = 2.0;
  CHECK(ss_check_params(2, 2, 1, L, sg, Ad, Qd, nullptr, nullptr, &where) == 0);
  const double a0n[2] = {0.0, NAN};
  CHECK(ss_check_params(2, 2, 1, L, sg, Ad, Qd, a0n, nullptr, &where) == SS_E_NAN);
  CHECK(ss_check_params(2, 2, 1, nullptr, sg, Ad, Qd, nullptr, nullptr, &where) == -2);
  CHECK(ss_check_params(2, 17, 1, L, sg, Ad, Qd, nullptr, nullptr, &where) == SS_E_LIMIT);

  // ---- the estimate, T = 3, N = 2, r = p = 1, f = (3, 4, 2).  Column 0 is exactly the common component: its
  //      variance is rejected by name.  Then one residual of 4 on it; column 1 has residuals +-1/2 and a missing
  //      entry.  Xl'Xl = 25 (a square: the Cholesky is exact), Xl'Y = 20, A = 4/5 by one division, U = (1.6, -1.2),
  //      Q = 2, P0 = Q / (1 - A^2) — these three to a few ulp.  Too few rows for the VAR are rejected.
  const double F[3] = {3.0, 4.0, 2.0}, Lz[2] = {2.0, 1.0};
  double Z[6] = {6.0, 8.0, 4.0, 3.5, 3.5, NAN};
  double sv[2], Ao[1], Qo[1], Po[1];
  where = -1;
  CHECK(ss_estimate(Z, 3, 2, 3, F, Lz, 1, 1, sv, Ao, Qo, Po, &where) == SS_E_SIGMA && where == 0);
  Z[1] += 4.0;
  CHECK(ss_estimate(Z, 3, 2, 3, F, Lz, 1, 1, sv, Ao, Qo, Po, &where) == 0);
  CHECK(sv[0] == 16.0 / 3.0 && sv[1] == 0.25);
  CHECK(Ao[0] == 4.0 / 5.0);
  CHECK(fabs(Qo[0] - 2.0) <= 1e-14 && fabs(Po[0] - 2.0 / 0.36) <= 1e-13);
  CHECK(ss_estimate(Z, 3, 2, 3, F, Lz, 1, 2, sv, Ao, Qo, Po, &where) == SS_E_VAR);   // T - p = 1 <= r p = 2

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
