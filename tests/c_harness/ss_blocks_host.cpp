// Stand-alone check of the factor blocks' host functions in
// csrc/dfm_ss_host.h with a plain C++ compiler: the checks of a block
// specification in the order they are made, the trivial specification, the
// offsets and the free mask, the check of a start's zeros, the gather and
// the deflation of the block-wise start, its per-block OLS against
// ss_var_ols on the block's own columns, and the low series' start on its
// free factors.  No HIP, nothing linked from the project.
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
  // ---- N = 4 series, blocks (2, 1): block 0 global, block 1 holds series 1 and 3
  const int32_t sizes[2] = {2, 1};
  const uint8_t member[8] = {1, 1, 1, 1, 0, 1, 0, 7};   // column-major N x 2; any non-zero byte is a member
  int64_t where = -1;
  CHECK(ss_blocks_check(2, sizes, member, 4, 3, &where) == SS_BLK_OK);
  CHECK(ss_blocks_check(2, nullptr, member, 4, 3, &where) == SS_BLK_NULL);
  CHECK(ss_blocks_check(2, sizes, nullptr, 4, 3, &where) == SS_BLK_NULL);
  CHECK(ss_blocks_check(0, sizes, member, 4, 3, &where) == SS_BLK_COUNT);
  CHECK(ss_blocks_check(17, sizes, member, 4, 3, &where) == SS_BLK_COUNT);
  const int32_t zero[2] = {2, 0};
  CHECK(ss_blocks_check(2, zero, member, 4, 2, &where) == SS_BLK_SIZE && where == 1);
  CHECK(ss_blocks_check(2, sizes, member, 4, 4, &where) == SS_BLK_SUM && where == 3);
  const uint8_t orphan[8] = {1, 1, 0, 1, 0, 1, 0, 1};
  CHECK(ss_blocks_check(2, sizes, orphan, 4, 3, &where) == SS_BLK_SERIES && where == 2);
  const uint8_t empty[8] = {1, 1, 1, 1, 0, 0, 0, 0};
  CHECK(ss_blocks_check(2, sizes, empty, 4, 3, &where) == SS_BLK_EMPTY && where == 1);
  // sixteen blocks of one are within the limit
  {
    int32_t ones[16];
    uint8_t all[32];
    for (int g = 0; g < 16; ++g) ones[g] = 1, all[2 * g] = all[2 * g + 1] = 1;
    CHECK(ss_blocks_check(16, ones, all, 2, 16, &where) == SS_BLK_OK);
    CHECK(!ss_blocks_trivial(16, all, 2));
  }
  // ---- no restriction: one block with every series
  const uint8_t every[4] = {1, 2, 1, 1}, notall[4] = {1, 0, 1, 1};
  CHECK(ss_blocks_trivial(1, every, 4) && !ss_blocks_trivial(1, notall, 4) && !ss_blocks_trivial(2, member, 4));
  // ---- the offsets and the free mask
  int off[3];
  ss_blocks_offsets(2, sizes, off);
  CHECK(off[0] == 0 && off[1] == 2 && off[2] == 3);
  uint16_t free[4];
  ss_blocks_free_mask(2, off, member, 4, free);
  CHECK(free[0] == 3 && free[1] == 7 && free[2] == 3 && free[3] == 7);
  // ---- a start's zeros: r = 3, p = 2
  double L[12] = {1, 2, 3, 4, 5, 6, 7, 8, 0, 9, 0, 10};   // N x r column-major: factor 2 restricted for series 0 and 2
  double A[18] = {0}, Q[9] = {0};
  for (int k = 0; k < 2; ++k) {   // A_k: the 2 x 2 block and the 1 x 1 block
    A[(k * 3 + 0) * 3 + 0] = 0.4, A[(k * 3 + 0) * 3 + 1] = 0.1, A[(k * 3 + 1) * 3 + 0] = -0.1, A[(k * 3 + 1) * 3 + 1] = 0.3;
    A[(k * 3 + 2) * 3 + 2] = 0.2;
  }
  Q[0] = Q[4] = Q[8] = 1.0, Q[1] = Q[3] = 0.2;
  int64_t row = -1, col = -1;
  CHECK(ss_blocks_check_start(4, 3, 2, L, A, Q, 2, off, free, &row, &col) == 0);
  L[2 * 4 + 2] = 1e-300;
  CHECK(ss_blocks_check_start(4, 3, 2, L, A, Q, 2, off, free, &row, &col) == 1 && row == 2 && col == 2);
  L[2 * 4 + 2] = -0.0;   // a negative zero is a zero
  CHECK(ss_blocks_check_start(4, 3, 2, L, A, Q, 2, off, free, &row, &col) == 0);
  A[(1 * 3 + 2) * 3 + 0] = 0.5;   // A_2[0, 2]: column 5 of the r x rp matrix
  CHECK(ss_blocks_check_start(4, 3, 2, L, A, Q, 2, off, free, &row, &col) == 2 && row == 0 && col == 5);
  A[(1 * 3 + 2) * 3 + 0] = 0.0;
  Q[2 * 3 + 1] = 0.1;             // Q[1, 2]
  CHECK(ss_blocks_check_start(4, 3, 2, L, A, Q, 2, off, free, &row, &col) == 3 && row == 1 && col == 2);
  // ---- the gather and the deflation: T = 3, block 1 (one factor) on its members 1 and 3
  {
    double R[12], Rg[6], F[9] = {0}, Lm[12] = {0};
    for (int e = 0; e < 12; ++e) R[e] = e + 1.0;
    CHECK(ss_blocks_gather(R, 3, 4, member + 4, Rg) == 2);
    for (int t = 0; t < 3; ++t) CHECK(Rg[t] == R[3 + t] && Rg[3 + t] == R[9 + t]);
    const double Fg[3] = {1.0, -1.0, 2.0}, Lg[2] = {0.5, 2.0};
    ss_blocks_deflate(R, 3, 4, member + 4, 2, 1, Fg, Lg, 2, F, Lm);
    for (int t = 0; t < 3; ++t) {
      CHECK(F[6 + t] == Fg[t] && F[t] == 0.0 && F[3 + t] == 0.0);
      CHECK(R[t] == t + 1.0 && R[6 + t] == 7.0 + t);                                   // not members
      CHECK(R[3 + t] == 4.0 + t - 0.5 * Fg[t] && R[9 + t] == 10.0 + t - 2.0 * Fg[t]);   // members
    }
    CHECK(Lm[8 + 1] == 0.5 && Lm[8 + 3] == 2.0 && Lm[8 + 0] == 0.0 && Lm[8 + 2] == 0.0 && Lm[1] == 0.0);
  }
  // ---- the block start's OLS: every block's A and Q are ss_var_ols of its own columns, placed
  // in its block of A_k and Q; the rest is zero; sigma^2 is ss_idio_var's
  {
    const int T = 12, N = 2, r = 3, p = 2;
    double F[36], Zm[24], Lm[6] = {0.5, -0.3, 0.2, 0.1, 0.0, 0.7};
    unsigned u = 12345u;
    for (int e = 0; e < 36; ++e) u = u * 1664525u + 1013904223u, F[e] = (double)(u >> 8) / (1u << 24) - 0.5;
    for (int e = 0; e < 24; ++e) u = u * 1664525u + 1013904223u, Zm[e] = (double)(u >> 8) / (1u << 24) - 0.5;
    Zm[5] = NAN;
    double sg[2], Ab[18], Qb[9], P0[36], sg1[2], A0[8], Q0[4], A1[2], Q1[1];
    CHECK(ss_blocks_estimate(Zm, T, N, T, F, Lm, r, p, 2, off, sg, Ab, Qb, P0, &where) == 0);
    CHECK(ss_idio_var(Zm, T, N, T, F, Lm, r, sg1, &where) == 0 && sg[0] == sg1[0] && sg[1] == sg1[1]);
    CHECK(ss_var_ols(F, T, 2, p, A0, Q0) == 0 && ss_var_ols(F + 2 * T, T, 1, p, A1, Q1) == 0);
    for (int k = 0; k < p; ++k)
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) {
          const double a = Ab[(k * 3 + j) * 3 + i];
          if (i < 2 && j < 2) CHECK(a == A0[(k * 2 + j) * 2 + i]);
          else if (i == 2 && j == 2) CHECK(a == A1[k]);
          else CHECK(a == 0.0);
        }
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) {
        const double q = Qb[j * 3 + i];
        if (i < 2 && j < 2) CHECK(q == Q0[j * 2 + i]);
        else if (i == 2 && j == 2) CHECK(q == Q1[0]);
        else CHECK(q == 0.0);
      }
    double Pw[36];
    CHECK(ss_stationary_cov(Ab, Qb, r, p, Pw) == 0);
    for (int e = 0; e < 36; ++e) CHECK(P0[e] == Pw[e]);
    // one block of all factors is ss_estimate
    const int off1[2] = {0, 3};
    double sg2[2], A2[18], Q2[9], P2[36], sg3[2], A3[18], Q3[9], P3[36];
    CHECK(ss_blocks_estimate(Zm, T, N, T, F, Lm, r, p, 1, off1, sg2, A2, Q2, P2, &where) == 0);
    CHECK(ss_estimate(Zm, T, N, T, F, Lm, r, p, sg3, A3, Q3, P3, &where) == 0);
    for (int e = 0; e < 18; ++e) CHECK(A2[e] == A3[e]);
    for (int e = 0; e < 9; ++e) CHECK(Q2[e] == Q3[e]);
    for (int e = 0; e < 36; ++e) CHECK(P2[e] == P3[e]);
    // too few rows for a block's VAR: T - p <= r_g p names the block
    double F6[18], Z6[12];
    for (int e = 0; e < 18; ++e) F6[e] = F[e];
    for (int e = 0; e < 12; ++e) Z6[e] = Zm[e] == Zm[e] ? Zm[e] : 0.25;
    CHECK(ss_blocks_estimate(Z6, 6, N, 6, F6, Lm, r, p, 2, off, sg, Ab, Qb, P0, &where) == SS_E_VAR && where == 0);
  }
  // ---- the low series' start on its free factors: r = 2, w = (1, 1), series 1 low and free on
  // factor 1 only: the scalar regression on the aggregate of factor 1, lambda_10 = 0 exactly
  {
    const double F[16] = {1, 2, 4, 3, 5, 8, 6, 7, 2, -1, 3, 0, 1, 4, -2, 5}, w2[2] = {1.0, 1.0};
    const uint8_t lo[2] = {0, 1};
    const uint16_t fr[2] = {3, 2};
    double Zm[16], L[4] = {9.0, 9.0, 9.0, 9.0}, sg[2] = {9.0, 9.0};
    for (int t = 0; t < 8; ++t) Zm[t] = 1.0, Zm[8 + t] = 0.1 * t * t - 1.0;
    Zm[8 + 3] = NAN;
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 2, w2, 2, lo, L, sg, &where, fr) == 0);
    double num = 0.0, den = 0.0, rss = 0.0;
    for (int t = 1; t < 8; ++t)
      if (t != 3) num += (F[8 + t] + F[8 + t - 1]) * Zm[8 + t], den += (F[8 + t] + F[8 + t - 1]) * (F[8 + t] + F[8 + t - 1]);
    for (int t = 1; t < 8; ++t)
      if (t != 3) rss += (Zm[8 + t] - num / den * (F[8 + t] + F[8 + t - 1])) * (Zm[8 + t] - num / den * (F[8 + t] + F[8 + t - 1]));
    CHECK(L[1] == 0.0 && fabs(L[3] - num / den) < 1e-14 && fabs(sg[1] - rss / 6.0) < 1e-14);
    CHECK(L[0] == 9.0 && L[2] == 9.0 && sg[0] == 9.0);
    // without the mask it is the regression on both aggregates
    double Lf[4] = {9.0, 9.0, 9.0, 9.0};
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 2, w2, 2, lo, Lf, sg, &where) == 0 && Lf[1] != 0.0);
    // two observed rows are enough for one free factor, not for two
    for (int t = 4; t < 8; ++t) Zm[8 + t] = NAN;
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 2, w2, 2, lo, L, sg, &where, fr) == 0);
    CHECK(ss_mf_start(Zm, 8, 2, 8, F, 2, w2, 2, lo, Lf, sg, &where) == SS_E_VAR && where == 1);
  }

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
