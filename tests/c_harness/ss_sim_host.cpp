// Stand-alone check of the simulation smoother's host arithmetic, and of the
// drivers' panels per pass, in csrc/dfm_ss_host.h with a plain C++ compiler: no
// HIP, nothing linked from the project.  The factor's inputs are integer-valued or dyadic, so every
// comparison is ==.
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
  // ---- ss_psd_cholesky: a rank-one 2 x 2, [[4,2],[2,1]] -> [[2,0],[1,0]]
  {
    const double C[4] = {4.0, 2.0, 2.0, 1.0};
    double R[4] = {-1.0, -1.0, -1.0, -1.0};
    ss_psd_cholesky(C, 2, R);
    CHECK(R[0] == 2.0 && R[1] == 0.0 && R[2] == 1.0 && R[3] == 0.0);
  }
  // ---- a zero matrix -> zero
  {
    const double C[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double R[9];
    for (double &v : R) v = -1.0;
    ss_psd_cholesky(C, 3, R);
    for (double v : R) CHECK(v == 0.0);
  }
  // ---- a full-rank 3 x 3: L = [[2,0,0],[1,3,0],[-1,0.5,4]], C = L L'
  {
    const double L[9] = {2.0, 0.0, 0.0, 1.0, 3.0, 0.0, -1.0, 0.5, 4.0};
    double C[9], R[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double v = 0.0;
        for (int k = 0; k < 3; ++k) v += L[i * 3 + k] * L[j * 3 + k];
        C[i * 3 + j] = v;
      }
    ss_psd_cholesky(C, 3, R);
    for (int e = 0; e < 9; ++e) CHECK(R[e] == L[e]);
  }
  // ---- a zero pivot in the middle: the first and third columns follow as usual.
  //      L = [[1,0,0],[2,0,0],[3,0,2]] -> C = [[1,2,3],[2,4,6],[3,6,13]]
  {
    const double C[9] = {1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 3.0, 6.0, 13.0};
    const double want[9] = {1.0, 0.0, 0.0, 2.0, 0.0, 0.0, 3.0, 0.0, 2.0};
    double R[9];
    ss_psd_cholesky(C, 3, R);
    for (int e = 0; e < 9; ++e) CHECK(R[e] == want[e]);
  }
  // ---- the count of normals: s + 2 r Tt
  CHECK(ss_sim_nz(11, 3, 6) == 72 && ss_sim_nz(12, 16, 32) == 416 && ss_sim_nz(1, 1, 1) == 3);
  CHECK(ss_sim_nz((int64_t)1 << 24, 16, 32) == 32 + 32 * ((int64_t)1 << 24));

  // ---- every rejection of ss_sim_check_args, and the calls it passes
  CHECK(ss_sim_check_args(1, true, true, 1, 0, 0) == 0);
  CHECK(ss_sim_check_args(70, true, true, 128, 3, 64) == 0);
  CHECK(ss_sim_check_args(SS_SIM_DMAX, true, true, SS_SIM_DMAX, 0, 0) == 0);
  CHECK(ss_sim_check_args(0, true, true, 1, 0, 0) == -2);                      // D < 1
  CHECK(ss_sim_check_args(-3, true, true, 1, 0, 0) == -2);
  CHECK(ss_sim_check_args(SS_SIM_DMAX + 1, true, true, SS_SIM_DMAX + 1, 0, 0) == -2);   // D > 2^24
  CHECK(ss_sim_check_args(5, false, true, 5, 0, 0) == -2);                     // no z
  CHECK(ss_sim_check_args(5, true, false, 5, 0, 0) == -2);                     // no output
  CHECK(ss_sim_check_args(5, true, true, 4, 0, 0) == -2);                      // ldz < D
  CHECK(ss_sim_check_args(5, true, true, 5, -1, 0) == -2);                     // horizon
  CHECK(ss_sim_check_args(5, true, true, 5, (1 << 20) + 1, 0) == -2);
  CHECK(ss_sim_check_args(5, true, true, 5, 0, -1) == -2);                     // pass_draws < 0

  // ---- draws per pass.  A caller's pass_draws holds, capped by D.
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 150, 64) == 64);
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 50, 64) == 50);
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 1, 1) == 1);
  // The workspace rule: 2^29 bytes over 8 (Tt s + 2 Tt r [+ nz]) per draw, whole waves.
  //   768 x (16 + 16) doubles = 196608 B per draw -> 2730 -> 2688 with z on the device
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 4096, 0, false) == 2688);
  //   + nz = 16 + 12288 doubles: 295040 B per draw -> 1819 -> 1792 with z from the host
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 4096, 0, true) == 1792);
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 4096, 0) == 1792);
  CHECK(ss_sim_draws_per_pass(768, 8, 16, 256, 0) == 256);                      // D below the rule
  CHECK(ss_sim_draws_per_pass(11, 3, 6, 73, 0) == 73);
  //   a draw larger than the half GB still gets a pass of its own; fewer than 64 are not rounded
  CHECK(ss_sim_draws_per_pass((int64_t)1 << 24, 16, 32, 5, 0) == 1);
  CHECK(ss_sim_draws_per_pass((int64_t)1 << 17, 16, 32, 100, 0, false) == 8);   // 2^29 / (8 x 2^17 x 64)

  // ---- panels per pass of the smoother and the EM: min(M, 65535, 2^29 / bytes per panel), at least 1
  CHECK(ss_panels_per_pass(3, 1000) == 3);                                      // M below both caps
  CHECK(ss_panels_per_pass(100000, 8) == 65535);                                // a launch grid's cap
  CHECK(ss_panels_per_pass(65535, 8) == 65535 && ss_panels_per_pass(65536, 8) == 65535);
  CHECK(ss_panels_per_pass(1000, (size_t)1 << 20) == 512);                      // the half GB
  CHECK(ss_panels_per_pass(1000, ((size_t)1 << 20) + 1) == 511);
  CHECK(ss_panels_per_pass(5, (size_t)1 << 30) == 1);                           // a panel larger than the half GB
  CHECK(ss_panels_per_pass(1, (size_t)1 << 30) == 1);
  //   T = 8, N = 4, r = 8, p = 4, horizon 4088 (tests/test_gpu_ss.py): a panel of the smoother keeps
  //   4096 + 4096 x 2112 + 64 + 32768 + 262144 + 2 doubles = 71598608 B -> 7 of M = 9 per pass
  CHECK(ss_panels_per_pass(9, (size_t)8 * (4096 + 4096 * 2112 + 64 + 32768 + 262144 + 2)) == 7);
  //   the EM's panel adds the M-step's rows (4096), the operand rows (512), the moments (2848) and its parameter
  //   block (4244), and 8 ints: 71692240 B -> 7 as well; at horizon 2040 (tests/test_gpu_ss_em.py) 35909584 B ->
  //   14 of M = 16
  CHECK(ss_panels_per_pass(9, (size_t)8 * (8949826 + 4096 + 512 + 2848 + 4244) + 32) == 7);
  CHECK(ss_panels_per_pass(16, (size_t)8 * (4096 + 2048 * 2112 + 64 + 16384 + 131072 + 2 + 11700) + 32) == 14);
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
