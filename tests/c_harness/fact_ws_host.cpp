// Stand-alone check of csrc/dfm_fact_ws.h with a plain C++ compiler: no HIP,
// nothing linked from the project.  Sweeps (T, nb, P, pz) and checks the
// factored solver's workspace layout against the sizes its consumers index
// and against the closed forms the solver used before the header existed.
#include "dfm_fact_ws.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                                                  \
  do {                                                                                               \
    if (!(cond)) {                                                                                   \
      if (failures < 20) std::printf("FAILED line %d (T=%d nb=%d P=%d pz=%d): %s\n", __LINE__, T, nb, P, pz, #cond); \
      ++failures;                                                                                    \
    }                                                                                                \
  } while (0)

int main() {
  using namespace dfm;
  const int Ts[] = {1, 15, 16, 17, 120, 121, 500, 2730, 2731, 4096};
  const int nbs[] = {1, 7, 64, 1250};
  const int Ps[] = {16, 32};
  const int pzs[] = {2, 12, 0};   // 0: pz = P
  for (int T : Ts)
    for (int nb : nbs)
      for (int P : Ps)
        for (int pzi : pzs) {
          const int pz = pzi ? pzi : P;
          const FactWsLayout L = fact_ws_layout(T, nb, P, pz);
          const size_t n = (size_t)nb, t = (size_t)T, zr = (size_t)z_rows(T), D = 8;
          CHECK(zr % 16 == 0 && zr >= t && zr < t + 16);
          // ascending, no overlap, each region at least what its consumer indexes
          CHECK(L.Z == 0);
          CHECK(L.Z < L.HZ && L.HZ < L.ab && L.ab < L.PF && L.PF < L.e2 && L.e2 < L.FV && L.FV < L.FtF &&
                L.FtF < L.total);
          CHECK(L.HZ - L.Z >= zr * n * pz * D);
          CHECK(L.ab - L.HZ >= t * n * pz * D);
          CHECK(L.PF - L.ab >= n * 32 * P * D);
          CHECK(L.e2 - L.PF >= n * t * 16 * D);
          CHECK(L.FV - L.e2 >= n * t * D);
          CHECK(L.FtF - L.FV >= n * 16 * P * D);
          CHECK(L.total - L.FtF >= 256 * D);
          // every region starts on a 16-byte boundary
          CHECK(L.Z % 16 == 0 && L.HZ % 16 == 0 && L.ab % 16 == 0 && L.PF % 16 == 0 && L.e2 % 16 == 0 &&
                L.FV % 16 == 0 && L.FtF % 16 == 0);
          // the total: the closed-form sum fact_workspace_bytes returned before, whatever pz
          const size_t nrb = (t + 63) / 64;
          const size_t old_total = (zr + t) * (n * P) * 8 + n * nrb * 2 * 32 * P * 8 + 4096 +
                                   (n * t * 17 + n * 16 * P + 256) * 8 + 4096;
          CHECK(L.total == old_total);
          CHECK(fact_ws_layout(T, nb, P, P).total == old_total);
          // the offsets: the solver's former pointer arithmetic (in doubles from the base), except that FV and FtF
          // move up 8 bytes where nb T is odd (there they sat 8 bytes off a 16-byte boundary)
          const size_t oHZ = zr * n * pz, oab = oHZ + t * n * pz, oPF = oab + n * nrb * 2 * 32 * P + 512,
                       oe2 = oPF + n * t * 16, oFV = oe2 + n * t, oFtF = oFV + n * 16 * P;
          const size_t pad = (n * t) % 2 ? 8 : 0;
          CHECK(L.HZ == oHZ * D && L.ab == oab * D && L.PF == oPF * D && L.e2 == oe2 * D);
          CHECK(L.FV == oFV * D + pad && L.FtF == oFtF * D + pad);
        }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
