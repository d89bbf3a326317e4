// dfm_fact_ws.h — the one statement of the factored solver's workspace
// (FactArgs::fws): where each region starts and how large the buffer is.
// Plain C++, no HIP: fact_workspace_bytes sizes the buffer from it,
// eig_run_fact2_t takes its pointers from it, and
// tests/c_harness/fact_ws_host.cpp checks it with a host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dfm {

// Z (the H.Z GEMM's B operand) has round_up(T, 16) rows, the pad rows zero, so
// the GEMM streams it with running DMA pointers and no k-tail clamp
inline int64_t z_rows(int T) { return ((int64_t)T + 15) / 16 * 16; }

// Byte offsets from the 16-byte-aligned base, in ascending order:
//   Z    z_rows(T) x nb pz doubles: replicate-major 16-row chunks (zrm_ix)
//   HZ   T x nb pz doubles, column-interleaved (rows gathered by idx)
//   ab   nb x 32 x P doubles: [a; cc] per replicate
//   PF   nb x T x 16 doubles: P'D F (T x r used)      } the middle Horner
//   e2   nb x T doubles: P'D^2 1                       } steps' operands
//   FV   nb x 16 x P doubles: F'V0                     } (boot_cheb_mid_kernel)
//   FtF  256 doubles: F'F (16 x 16, shared)            }
struct FactWsLayout {
  size_t Z, HZ, ab, PF, e2, FV, FtF, total;
};
// P: the block width the buffer is sized for (16 or 32); pz <= P, even: the
// columns per replicate that Z and HZ hold in this solve (p rounded up to
// even).  Z and HZ are packed at pz, so the regions behind them start where
// the solve's own column count puts them; total does not depend on pz and is
// what fact_workspace_bytes(T, nb, P) has always returned.
inline FactWsLayout fact_ws_layout(int T, int nb, int P, int pz) {
  const size_t D = sizeof(double), n = (size_t)nb, t = (size_t)T;
  // ab is sized by the 64-row block count of a per-row-block path that no
  // longer exists (2 x 32 x P doubles per block, + 512); its consumers index
  // nb x 32 x P.  Kept: shrinking it would move every region behind it.
  const size_t nrb = (t + 63) / 64;
  const size_t ab_bytes = (n * nrb * 2 * 32 * P + 512) * D;
  FactWsLayout L;
  L.Z = 0;
  L.HZ = L.Z + (size_t)z_rows(T) * n * pz * D;
  L.ab = L.HZ + t * n * pz * D;
  L.PF = L.ab + ab_bytes;
  L.e2 = L.PF + n * t * 16 * D;
  // e2 holds nb T doubles; FV starts at the next 16-byte boundary (an odd
  // nb T used to leave FV and FtF 8 bytes short of one; the slack covers it)
  L.FV = L.e2 + ((n * t + 1) & ~(size_t)1) * D;
  L.FtF = L.FV + n * 16 * P * D;
  // the end of FtF (256 doubles), the columns Z and HZ leave unused at this pz,
  // and 4096 bytes of slack less e2's pad: the regions at pz = P, + 4096
  L.total = L.FtF + 256 * D + (size_t)(z_rows(T) + T) * n * (P - pz) * D + 4096 - (L.FV - L.e2 - n * t * D);
  return L;
}

}  // namespace dfm
