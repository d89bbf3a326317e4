// Stand-alone check of the EM's host functions in csrc/dfm_ss_host.h with a
// plain C++ compiler: the stopping rule, the spec's defaults and the argument
// rejections.  No HIP, nothing linked from the project.
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
  // ---- the criterion: (ll - prev) / ((|ll| + |prev|) / 2), dyadic inputs
  CHECK(ss_em_criterion(-3.0, -5.0) == 0.5);        // 2 / 4
  CHECK(ss_em_criterion(-5.0, -3.0) == -0.5);       // a decrease is negative
  CHECK(ss_em_criterion(1.0, -1.0) == 2.0);
  CHECK(ss_em_criterion(0.0, 0.0) == 0.0);          // a zero denominator
  CHECK(ss_em_criterion(-4.0, -4.0) == 0.0);
  // ---- the rule, at and on both sides of tol; tol = 0 never stops
  const double tol = 0.125;
  CHECK(ss_em_converged(0.0625, tol) && !ss_em_converged(0.125, tol) && !ss_em_converged(0.25, tol));
  CHECK(ss_em_converged(ss_em_criterion(-15.0, -17.0), 0.1875) == true);    // c = 1/8 < 3/16
  CHECK(ss_em_converged(ss_em_criterion(-15.0, -17.0), 0.125) == false);    // c = tol
  CHECK(ss_em_converged(-0.5, tol));                // a decrease stops too (Banbura-Modugno)
  CHECK(ss_em_converged(ss_em_criterion(0.0, 0.0), tol));
  CHECK(!ss_em_converged(0.0, 0.0) && !ss_em_converged(-1.0, 0.0) && !ss_em_converged(1e-300, 0.0));
  CHECK(!ss_em_converged(NAN, tol));
  // ---- the defaults
  int mi = -1;
  double tl = -1.0;
  CHECK(ss_em_defaults(-1, -1.0, 0, &mi, &tl) == 0 && mi == 100 && tl == 1e-4);
  CHECK(ss_em_defaults(0, 0.0, 3, &mi, &tl) == 0 && mi == 0 && tl == 0.0);
  CHECK(ss_em_defaults(7, 0.5, 0, &mi, &tl) == 0 && mi == 7 && tl == 0.5);
  CHECK(ss_em_defaults(7, NAN, 0, &mi, &tl) == -2);
  CHECK(ss_em_defaults(7, 0.5, -1, &mi, &tl) == -2);
  CHECK(ss_em_defaults(SS_EM_ITER_CAP + 1, 0.5, 0, &mi, &tl) == -2);
  // ---- the batch's layout
  CHECK(ss_em_check_args(true, 3, 10, 4, 10, 40, true, 1) == 0);
  CHECK(ss_em_check_args(true, 3, 10, 4, 12, 50, true, 3) == 0);
  CHECK(ss_em_check_args(false, 0, 0, 0, 0, 0, true, 1) == 0);      // an empty batch
  CHECK(ss_em_check_args(true, 3, 10, 4, 10, 40, true, 2) == -2);   // n_start neither 1 nor M
  CHECK(ss_em_check_args(true, 3, 10, 4, 10, 40, false, 1) == -2);
  CHECK(ss_em_check_args(false, 3, 10, 4, 10, 40, true, 1) == -2);
  CHECK(ss_em_check_args(true, 3, 1, 4, 1, 4, true, 1) == -2);      // T < 2
  CHECK(ss_em_check_args(true, 3, 10, 0, 10, 40, true, 1) == -2);
  CHECK(ss_em_check_args(true, 3, 10, 4, 9, 40, true, 1) == -2);    // ldx < T
  CHECK(ss_em_check_args(true, 3, 10, 4, 10, 39, true, 1) == -2);   // stride < ldx N
  CHECK(ss_em_check_args(true, -1, 10, 4, 10, 40, true, 1) == -2);
  // ---- a start: the smoother's checks, then Q positive definite
  const double L[4] = {1.0, 2.0, 3.0, 4.0}, Ad[4] = {0.5, 0.0, 0.0, 0.5};   // N = 2, r = 2, p = 1
  double sg[2] = {1.0, 2.0}, Q[4] = {2.0, 1.0, 1.0, 2.0};
  int64_t where = -1;
  CHECK(ss_em_check_start(2, 2, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == 0);
  Q[0] = 4.0, Q[1] = Q[2] = 2.0, Q[3] = 1.0;   // singular: the second pivot is 1 - 1 exactly
  CHECK(ss_em_check_start(2, 2, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == SS_E_SINGULAR);
  Q[1] = Q[2] = 3.0;   // indefinite
  CHECK(ss_em_check_start(2, 2, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == SS_E_SINGULAR);
  Q[0] = 2.0, Q[1] = Q[2] = 1.0, Q[3] = 2.0;
  sg[0] = -1.0;
  CHECK(ss_em_check_start(2, 2, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == SS_E_SIGMA && where == 0);
  sg[0] = 1.0;
  Q[3] = NAN;
  CHECK(ss_em_check_start(2, 2, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == SS_E_NAN);
  Q[3] = 2.0;
  CHECK(ss_em_check_start(2, 17, 1, L, sg, Ad, Q, nullptr, nullptr, &where) == SS_E_LIMIT);
  // ---- a column without an observed entry: two panels of T = 3, N = 2, ldx = 4, stride = 9
  double X[18];
  for (double &v : X) v = 1.0;
  int64_t pb = -1, col = -1;
  CHECK(!ss_em_empty_column(X, 2, 3, 2, 4, 9, &pb, &col));
  X[3] = NAN;   // padding between the columns is not read
  X[9 + 4] = X[9 + 5] = NAN;
  CHECK(!ss_em_empty_column(X, 2, 3, 2, 4, 9, &pb, &col));
  X[9 + 6] = NAN;
  CHECK(ss_em_empty_column(X, 2, 3, 2, 4, 9, &pb, &col) && pb == 1 && col == 1);

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
